// A stand-alone check of csrc/kernels/bk_dispatch.hpp, for
// tests/test_native_abi_cpu.py (which builds it with g++ under ASan / UBSan
// and runs it): every code in range reaches its one instantiation, once, and
// every other code is kBadArgument without a call.  The header is plain C++:
// this needs neither hipcc nor the library.
#include <climits>
#include <cstdio>

#include "../csrc/kernels/bk_dispatch.hpp"

using namespace bk;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      ++failures;                                                \
    }                                                            \
  } while (0)

int main() {
  static_assert(kBadArgument == 1 && kOk == 0, "status codes of beekern.h");

  // dispatch_op: the constant is the code, f runs once, its value comes back
  for (int op = 0; op < 7; ++op) {
    int calls = 0, got = -1;
    const int rc = dispatch_op<7>(op, [&](auto c) {
      static_assert(decltype(c)::value >= 0 && decltype(c)::value < 7, "only codes in range are instantiated");
      ++calls;
      got = decltype(c)::value;
      return 100 + decltype(c)::value;
    });
    CHECK(calls == 1 && got == op && rc == 100 + op);
  }
  for (int op : {-1, 7, INT_MAX, INT_MIN}) {
    int calls = 0;
    CHECK(dispatch_op<7>(op, [&](auto) { return ++calls, 0; }) == 1);
    CHECK(calls == 0);
  }

  // dispatch_flag: the matching tag, once
  for (int b = 0; b < 2; ++b) {
    int calls_true = 0, calls_false = 0;
    const int rc = dispatch_flag(b != 0, [&](auto flag) {
      if constexpr (decltype(flag)::value) ++calls_true;
      else ++calls_false;
      return decltype(flag)::value ? 7 : 8;
    });
    CHECK(calls_true == b && calls_false == 1 - b && rc == (b ? 7 : 8));
  }

  // dispatch_dtype: each listed code reaches its element type
  auto type_of = [](int dtype, int* calls, unsigned long* size, bool* is_f32, bool* is_f64, bool* is_bf16, bool* is_bool) {
    return dispatch_dtype<float, double, unsigned short, unsigned char>(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      ++*calls;
      *size = sizeof(T);
      *is_f32 = std::is_same<T, float>::value;
      *is_f64 = std::is_same<T, double>::value;
      *is_bf16 = std::is_same<T, unsigned short>::value;
      *is_bool = std::is_same<T, unsigned char>::value;
      return 40 + DTypeOf<T>::value;
    });
  };
  struct Want { int code; unsigned long size; int which; };
  for (const Want w : {Want{kF32, 4, 0}, Want{kF64, 8, 1}, Want{kBF16, 2, 2}, Want{kBool, 1, 3}}) {
    int calls = 0;
    unsigned long size = 0;
    bool is[4] = {false, false, false, false};
    const int rc = type_of(w.code, &calls, &size, &is[0], &is[1], &is[2], &is[3]);
    CHECK(calls == 1 && size == w.size && rc == 40 + w.code);
    for (int i = 0; i < 4; ++i) CHECK(is[i] == (i == w.which));
  }
  CHECK(kF32 == 0 && kF64 == 1 && kBF16 == 2 && kBool == 6);
  // a code outside the list: f16, i32, i64, and -- for a list without it -- bool
  for (int dtype : {3, 4, 5, 6, -1, 7, INT_MAX}) {
    int calls = 0;
    CHECK((dispatch_dtype<float, double, unsigned short>(dtype, [&](auto) { return ++calls, 0; })) == 1);
    CHECK(calls == 0);
  }
  for (int dtype : {3, 4, 5, -1}) {
    int calls = 0;
    unsigned long size = 0;
    bool is[4];
    CHECK(type_of(dtype, &calls, &size, &is[0], &is[1], &is[2], &is[3]) == 1);
    CHECK(calls == 0);
  }

  if (failures) return 1;
  printf("dispatch ok\n");
  return 0;
}
