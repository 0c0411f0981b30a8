// Elementwise kernels (square, unary math, binary arithmetic, casts, bool -> float).
//
// HBM-bound: every lane moves 16 bytes per access (f64x2 / f32x4 / bf16x8,
// Guideline 13), non-temporal for arrays past the Infinity Cache
// (bk_common.hpp ld16/st16), grid-stride over <= 64 blocks per CU.  bf16 math runs in f32
// and rounds once on store.  `numpy.square` of the benchmark payload
// (`examples/benchmark-numpy.py:21`) is kUnarySquare on f64.
#include "bk_binary_op.hpp"  // BinaryOp and binary<OP>, shared with axis.hip
#include "bk_common.hpp"

namespace bk {

enum UnaryOp : int {
  kUnarySquare = 0, kUnaryAbs, kUnaryNeg, kUnarySqrt, kUnaryExp, kUnaryLog, kUnaryRelu,
  kUnarySin, kUnaryCos, kUnaryTanh, kUnarySigmoid, kUnaryCopy, kUnaryCount
};

template <typename T> struct Elem;  // storage <-> compute type
template <> struct Elem<float> {
  using C = float;
  __device__ static C load(float v) { return v; }
  __device__ static float store(C v) { return v; }
};
template <> struct Elem<double> {
  using C = double;
  __device__ static C load(double v) { return v; }
  __device__ static double store(C v) { return v; }
};
template <> struct Elem<uint16_t> {  // bf16 bits
  using C = float;
  __device__ static C load(uint16_t v) { return bf16_bits_to_float(v); }
  __device__ static uint16_t store(C v) { return float_to_bf16_bits(v); }
};

template <int OP, typename C>
__device__ __forceinline__ C unary(C x) {
  if constexpr (OP == kUnarySquare) return x * x;
  // numpy.absolute: the sign bit cleared, so abs(-0.0) = +0.0 and a NaN comes out positive
  else if constexpr (OP == kUnaryAbs) return fabs(x);
  else if constexpr (OP == kUnaryNeg) return -x;
  else if constexpr (OP == kUnarySqrt) return sqrt(x);
  else if constexpr (OP == kUnaryExp) return exp(x);
  else if constexpr (OP == kUnaryLog) return log(x);
  // numpy.maximum(x, 0): NaN stays NaN (as kBinMax); zeros and negatives give +0.0
  else if constexpr (OP == kUnaryRelu) return (x > C(0) || x != x) ? x : C(0);
  else if constexpr (OP == kUnarySin) return sin(x);
  else if constexpr (OP == kUnaryCos) return cos(x);
  else if constexpr (OP == kUnaryTanh) return tanh(x);
  else if constexpr (OP == kUnarySigmoid) return C(1) / (C(1) + exp(-x));
  else return x;
}

template <typename T, int OP, bool NT>
__global__ __launch_bounds__(256) void unary_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n) {
  using E = Elem<T>;
  using V = V16<T>;
  constexpr int N = V::N, U = kStreamUnroll;
  const int64_t nvec = n / N;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const V* xv = reinterpret_cast<const V*>(x);
  V* yv = reinterpret_cast<V*>(y);
  // block-contiguous chunks of U*256 vectors: each load instruction of a wave
  // covers 1 KiB contiguous and a block's U instructions one 16 KiB span
  const int64_t chunk = (int64_t)U * blockDim.x;
  const int64_t nfull = nvec / chunk;
  for (int64_t cb = blockIdx.x; cb < nfull; cb += gridDim.x) {
    const int64_t base = cb * chunk + threadIdx.x;
    V a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = ld16<NT>(xv + base + u * blockDim.x);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < N; ++j) a[u].v[j] = E::store(unary<OP>(E::load(a[u].v[j])));
#pragma unroll
    for (int u = 0; u < U; ++u) st16<NT>(yv + base + u * blockDim.x, a[u]);
  }
  for (int64_t i = nfull * chunk + tid; i < nvec; i += stride) {
    V a = xv[i];
#pragma unroll
    for (int j = 0; j < N; ++j) a.v[j] = E::store(unary<OP>(E::load(a.v[j])));
    yv[i] = a;
  }
  for (int64_t k = nvec * N + tid; k < n; k += stride) y[k] = E::store(unary<OP>(E::load(x[k])));
}

// y = op(a, b) with b an array (B_SCALAR=false) or a scalar (B_SCALAR=true);
// REVERSED swaps the operands for scalar ops (s - x, s / x, ...).
template <typename T, int OP, bool B_SCALAR, bool REVERSED, bool NT>
__global__ __launch_bounds__(256) void binary_kernel(const T* __restrict__ a, const T* __restrict__ b, double s,
                                                     T* __restrict__ y, int64_t n) {
  using E = Elem<T>;
  using C = typename E::C;
  using V = V16<T>;
  constexpr int N = V::N;
  constexpr int U = kStreamUnroll;
  const C sc = (C)s;
  const int64_t nvec = n / N;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const V* av = reinterpret_cast<const V*>(a);
  const V* bv = reinterpret_cast<const V*>(b);
  V* yv = reinterpret_cast<V*>(y);
  auto apply = [&](V& va, const V& vb) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const C lhs = E::load(va.v[j]);
      const C rhs = B_SCALAR ? sc : E::load(vb.v[j]);
      va.v[j] = E::store(REVERSED ? binary<OP>(rhs, lhs) : binary<OP>(lhs, rhs));
    }
  };
  const int64_t chunk = (int64_t)U * blockDim.x;
  const int64_t nfull = nvec / chunk;
  for (int64_t cb = blockIdx.x; cb < nfull; cb += gridDim.x) {
    const int64_t base = cb * chunk + threadIdx.x;
    V va[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      va[u] = ld16<NT>(av + base + u * blockDim.x);
      if constexpr (!B_SCALAR) vb[u] = ld16<NT>(bv + base + u * blockDim.x);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) apply(va[u], vb[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) st16<NT>(yv + base + u * blockDim.x, va[u]);
  }
  for (int64_t i = nfull * chunk + tid; i < nvec; i += stride) {
    V va = av[i], vb;
    if constexpr (!B_SCALAR) vb = bv[i];
    apply(va, vb);
    yv[i] = va;
  }
  for (int64_t k = nvec * N + tid; k < n; k += stride) {
    const C lhs = E::load(a[k]);
    const C rhs = B_SCALAR ? sc : E::load(b[k]);
    y[k] = E::store(REVERSED ? binary<OP>(rhs, lhs) : binary<OP>(lhs, rhs));
  }
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void cast_kernel(const TI* __restrict__ x, TO* __restrict__ y, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if constexpr (std::is_same<TI, double>::value && std::is_same<TO, uint16_t>::value)
      y[i] = double_to_bf16_bits(x[i]);
    else
      y[i] = Elem<TO>::store((typename Elem<TO>::C)Elem<TI>::load(x[i]));
  }
}

// kBool -> f32 / f64: any non-zero byte is 1.0 (16 mask bytes per lane and load)
template <typename TO>
__global__ __launch_bounds__(256) void bool_cast_kernel(const uint8_t* __restrict__ x, TO* __restrict__ y, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nvec = n / 16;
  for (int64_t i = tid; i < nvec; i += stride) {
    const V16<uint8_t> m = reinterpret_cast<const V16<uint8_t>*>(x)[i];
    constexpr int N = V16<TO>::N;
#pragma unroll
    for (int q = 0; q < 16 / N; ++q) {
      V16<TO> o;
#pragma unroll
      for (int j = 0; j < N; ++j) o.v[j] = m.v[q * N + j] != 0 ? TO(1) : TO(0);
      reinterpret_cast<V16<TO>*>(y)[i * (16 / N) + q] = o;
    }
  }
  for (int64_t k = nvec * 16 + tid; k < n; k += stride) y[k] = x[k] != 0 ? TO(1) : TO(0);
}

__global__ __launch_bounds__(256) void fill_kernel(uint8_t* __restrict__ y, int64_t nbytes, uint64_t pattern,
                                                   int pattern_bytes) {
  // pattern_bytes in {1,2,4,8}; 16-B stores for the bulk.
  uint64_t p = pattern;
  if (pattern_bytes == 1) p = (p & 0xff) * 0x0101010101010101ull;
  if (pattern_bytes == 2) p = (p & 0xffff) * 0x0001000100010001ull;
  if (pattern_bytes == 4) p = (p & 0xffffffffull) | ((p & 0xffffffffull) << 32);
  const uint4 v = make_uint4((uint32_t)p, (uint32_t)(p >> 32), (uint32_t)p, (uint32_t)(p >> 32));
  const int64_t nvec = nbytes / 16;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = tid; i < nvec; i += stride) reinterpret_cast<uint4*>(y)[i] = v;
  for (int64_t i = nvec * 16 + tid; i < nbytes; i += stride) y[i] = (uint8_t)(p >> (8 * (i % 8)));
}

}  // namespace bk

using namespace bk;

// (contracts of the entry points: beekern.h)
BK_API int bk_unary(int op, int dtype, const void* x, void* y, int64_t n, hipStream_t stream) {
  if (!x || !y || n < 0 || op < 0 || op >= kUnaryCount) return kBadArgument;
  if (n == 0) return kOk;
  return dispatch_dtype<float, double, uint16_t>(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    const unsigned g = stream_grid((n + V16<T>::N - 1) / V16<T>::N, 256);
    return dispatch_op<kUnaryCount>(op, [&](auto opc) {
      return dispatch_flag(stream_nt(n * (int64_t)sizeof(T)), [&](auto nt) {
        unary_kernel<T, decltype(opc)::value, decltype(nt)::value><<<g, 256, 0, stream>>>((const T*)x, (T*)y, n);
        return launch_status();
      });
    });
  });
}

BK_API int bk_binary(int op, int dtype, int mode, const void* a, const void* b, double scalar, void* y, int64_t n,
                     hipStream_t stream) {
  if (!a || !y || n < 0 || op < 0 || op >= kBinCount || mode < 0 || mode > 2 || (mode == 0 && !b))
    return kBadArgument;
  if (n == 0) return kOk;
  return dispatch_dtype<float, double, uint16_t>(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    const unsigned g = stream_grid((n + V16<T>::N - 1) / V16<T>::N, 256);
    return dispatch_op<kBinCount>(op, [&](auto opc) {
      // mode 0: b is an array; 1: the scalar on the right; 2: the scalar on the left
      return dispatch_flag(mode == 0, [&](auto b_array) {
        return dispatch_flag(mode != 2, [&](auto a_left) {
          return dispatch_flag(stream_nt(n * (int64_t)sizeof(T)), [&](auto nt) {
            constexpr bool BS = !decltype(b_array)::value, REV = !decltype(a_left)::value;
            if constexpr (BS || !REV)  // (no mode swaps two arrays)
              binary_kernel<T, decltype(opc)::value, BS, REV, decltype(nt)::value>
                  <<<g, 256, 0, stream>>>((const T*)a, (const T*)b, scalar, (T*)y, n);
            return launch_status();
          });
        });
      });
    });
  });
}

BK_API int bk_cast(int src_dtype, int dst_dtype, const void* x, void* y, int64_t n, hipStream_t stream) {
  if (!x || !y || n < 0) return kBadArgument;
  if (n == 0) return kOk;
  if (src_dtype == kBool && (dst_dtype == kF32 || dst_dtype == kF64)) {
    const unsigned gb = stream_grid((n + 15) / 16, 256);
    if (dst_dtype == kF32) bool_cast_kernel<float><<<gb, 256, 0, stream>>>((const uint8_t*)x, (float*)y, n);
    else bool_cast_kernel<double><<<gb, 256, 0, stream>>>((const uint8_t*)x, (double*)y, n);
    return launch_status();
  }
  const unsigned g = stream_grid(n, 256);
#define BK_CAST(TI, TO) cast_kernel<TI, TO><<<g, 256, 0, stream>>>((const TI*)x, (TO*)y, n)
  if (src_dtype == kF32 && dst_dtype == kBF16) BK_CAST(float, uint16_t);
  else if (src_dtype == kBF16 && dst_dtype == kF32) BK_CAST(uint16_t, float);
  else if (src_dtype == kF64 && dst_dtype == kF32) BK_CAST(double, float);
  else if (src_dtype == kF32 && dst_dtype == kF64) BK_CAST(float, double);
  else if (src_dtype == kF64 && dst_dtype == kBF16) BK_CAST(double, uint16_t);
  else if (src_dtype == kBF16 && dst_dtype == kF64) BK_CAST(uint16_t, double);
  else return kBadArgument;
#undef BK_CAST
  return launch_status();
}

BK_API int bk_fill(void* y, int64_t nbytes, uint64_t pattern, int pattern_bytes, hipStream_t stream) {
  if (!y || nbytes < 0 || !(pattern_bytes == 1 || pattern_bytes == 2 || pattern_bytes == 4 || pattern_bytes == 8))
    return kBadArgument;
  if (nbytes == 0) return kOk;
  fill_kernel<<<stream_grid((nbytes + 15) / 16, 256), 256, 0, stream>>>((uint8_t*)y, nbytes, pattern, pattern_bytes);
  return launch_status();
}
