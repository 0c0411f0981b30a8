// int64 arrays: arithmetic, comparisons, whole-array reductions, casts, and the
// integer-valued random draws (integers, poisson, binomial, geometric).
//
// Every element is int64_t.  The streaming kernels move 16 bytes (two
// elements) per lane and access, non-temporal past the Infinity Cache
// (bk_common.hpp).  An int64 array may start 8 bytes off a 16-byte boundary (a
// view from an odd element): when every operand does, the first element is
// handled alone and the vectors start behind it; operands that disagree take
// the element-wise tail loop for the whole array.
//
// Arithmetic wraps in two's complement (computed in uint64_t); floor_divide
// and remainder follow Python's sign rule, give 0 for a zero divisor, and
// INT64_MIN // -1 = INT64_MIN, INT64_MIN % -1 = 0: numpy's answers on x86-64.
//
// No workgroup waits for another: the reduction folds by completion ticket
// (bk_ticket.hpp), on the scalar reductions' own workspace.
#include <cmath>

#include "bk_common.hpp"
#include "bk_philox.hpp"
#include "bk_ticket.hpp"

namespace bk {
namespace integer {

using I64Vec = V16<int64_t>;

constexpr int64_t kI64Min = INT64_MIN, kI64Max = INT64_MAX;

enum IntBinaryOp : int { kIAdd = 0, kISub, kIMul, kIFloorDiv, kIRem, kIMax, kIMin, kIBinCount };
enum IntCompareOp : int { kILt = 0, kILe, kIGt, kIGe, kIEq, kINe, kICmpCount };  // bk_compare's codes
enum IntReduceOp : int { kIRedSum = 0, kIRedMax, kIRedMin, kIRedCount };

template <int OP>
__device__ __forceinline__ int64_t ibinary(int64_t a, int64_t b) {
  if constexpr (OP == kIAdd) return (int64_t)((uint64_t)a + (uint64_t)b);
  else if constexpr (OP == kISub) return (int64_t)((uint64_t)a - (uint64_t)b);
  else if constexpr (OP == kIMul) return (int64_t)((uint64_t)a * (uint64_t)b);
  else if constexpr (OP == kIFloorDiv) {
    if (b == 0) return 0;
    if (b == -1) return (int64_t)(0ull - (uint64_t)a);  // INT64_MIN stays: a / -1 would overflow
    const int64_t q = a / b, r = a - q * b;
    return (r != 0 && ((r < 0) != (b < 0))) ? q - 1 : q;
  } else if constexpr (OP == kIRem) {
    if (b == 0 || b == -1) return 0;  // (a % -1 overflows for INT64_MIN)
    const int64_t r = a % b;
    return (r != 0 && ((r < 0) != (b < 0))) ? r + b : r;
  } else if constexpr (OP == kIMax) return a > b ? a : b;
  else return a < b ? a : b;
}

template <int OP>
__device__ __forceinline__ bool icmp(int64_t a, int64_t b) {
  if constexpr (OP == kILt) return a < b;
  else if constexpr (OP == kILe) return a <= b;
  else if constexpr (OP == kIGt) return a > b;
  else if constexpr (OP == kIGe) return a >= b;
  else if constexpr (OP == kIEq) return a == b;
  else return a != b;
}

// How a launch splits [0, n): `head` elements alone, nvec vectors behind them,
// the rest alone.  Every operand 16-byte aligned: head 0.  Every operand 8
// bytes off: head 1.  Operands that disagree: no vectors.
struct Split {
  int64_t head, nvec;
};
inline Split split_of(int64_t n, std::initializer_list<const void*> ptrs) {
  int off = -1;
  for (const void* p : ptrs) {
    if (!p) continue;
    const int o = (int)((uintptr_t)p & 15);
    if (o != 0 && o != 8) return Split{0, 0};  // (not an int64 pointer: the tail loop faults no worse than a load)
    if (off >= 0 && o != off) return Split{0, 0};
    off = o;
  }
  const int64_t head = (off == 8 && n > 0) ? 1 : 0;
  return Split{head, (n - head) / 2};
}

// y = a OP b; B_SCALAR: b is the scalar s; REVERSED: s OP a.  y may be a or b
// (no __restrict__): a lane reads the elements it writes, nobody else's.
template <int OP, bool B_SCALAR, bool REVERSED, bool NT>
__global__ __launch_bounds__(256) void int_binary_kernel(const int64_t* a, const int64_t* b, int64_t s, int64_t* y,
                                                         int64_t n, Split sp) {
  constexpr int U = kStreamUnroll;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  auto one = [&](int64_t lhs, int64_t rhs) { return REVERSED ? ibinary<OP>(rhs, lhs) : ibinary<OP>(lhs, rhs); };
  auto apply = [&](I64Vec& va, const I64Vec& vb) {
#pragma unroll
    for (int j = 0; j < 2; ++j) va.v[j] = one(va.v[j], B_SCALAR ? s : vb.v[j]);
  };
  if (tid < sp.head) y[tid] = one(a[tid], B_SCALAR ? s : b[tid]);
  const I64Vec* av = reinterpret_cast<const I64Vec*>(a + sp.head);
  const I64Vec* bv = reinterpret_cast<const I64Vec*>(b + sp.head);
  I64Vec* yv = reinterpret_cast<I64Vec*>(y + sp.head);
  const int64_t chunk = (int64_t)U * blockDim.x;
  const int64_t nfull = sp.nvec / chunk;
  for (int64_t cb = blockIdx.x; cb < nfull; cb += gridDim.x) {
    const int64_t base = cb * chunk + threadIdx.x;
    I64Vec va[U], vb[U];
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
  for (int64_t i = nfull * chunk + tid; i < sp.nvec; i += stride) {
    I64Vec va = av[i], vb;
    if constexpr (!B_SCALAR) vb = bv[i];
    apply(va, vb);
    yv[i] = va;
  }
  for (int64_t k = sp.head + sp.nvec * 2 + tid; k < n; k += stride) y[k] = one(a[k], B_SCALAR ? s : b[k]);
}

// mask_out[i] = a[i] OP b[i] (or s) as a 0 / 1 byte.  A lane's vector yields
// two mask bytes: one 2-byte store where the mask behind the head is 2-byte
// aligned (Y2), two byte stores otherwise.
template <int OP, bool SCALAR, bool NT, bool Y2>
__global__ __launch_bounds__(256) void int_compare_kernel(const int64_t* __restrict__ a, const int64_t* __restrict__ b,
                                                          int64_t s, uint8_t* __restrict__ y, int64_t n, Split sp) {
  constexpr int U = kStreamUnroll;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid < sp.head) y[tid] = icmp<OP>(a[tid], SCALAR ? s : b[tid]) ? 1 : 0;
  const I64Vec* av = reinterpret_cast<const I64Vec*>(a + sp.head);
  const I64Vec* bv = reinterpret_cast<const I64Vec*>(b + sp.head);
  uint8_t* ym = y + sp.head;
  auto put = [&](int64_t i, const I64Vec& va, const I64Vec& vb) {
    const uint8_t m0 = icmp<OP>(va.v[0], SCALAR ? s : vb.v[0]) ? 1 : 0;
    const uint8_t m1 = icmp<OP>(va.v[1], SCALAR ? s : vb.v[1]) ? 1 : 0;
    if constexpr (Y2) {
      *reinterpret_cast<uint16_t*>(ym + 2 * i) = (uint16_t)(m0 | (m1 << 8));
    } else {
      ym[2 * i] = m0;
      ym[2 * i + 1] = m1;
    }
  };
  int64_t i = tid;
  for (; i + (U - 1) * stride < sp.nvec; i += U * stride) {
    I64Vec va[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      va[u] = ld16<NT>(av + i + u * stride);
      if constexpr (!SCALAR) vb[u] = ld16<NT>(bv + i + u * stride);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) put(i + u * stride, va[u], vb[u]);
  }
  for (; i < sp.nvec; i += stride) {
    I64Vec va = av[i], vb;
    if constexpr (!SCALAR) vb = bv[i];
    put(i, va, vb);
  }
  for (int64_t k = sp.head + sp.nvec * 2 + tid; k < n; k += stride) y[k] = icmp<OP>(a[k], SCALAR ? s : b[k]) ? 1 : 0;
}

// ---- whole-array sum / max / min ----------------------------------------------------
// One launch on BK_WS_REDUCE: its kRedMaxBlocks 8-byte partial slots hold int64
// partials here, the ticket sits behind them.  Integer addition (wrapping) and
// max / min are associative and commutative: the result is exact whatever the grid.
constexpr int kIntRedVecsPerLane = 4;  // vectors a lane has before the grid grows: a block spans 256 * 4 * 2 elements

template <int OP> __device__ __forceinline__ int64_t ired_init() {
  if constexpr (OP == kIRedMax) return kI64Min;
  else if constexpr (OP == kIRedMin) return kI64Max;
  else return 0;
}
template <int OP> __device__ __forceinline__ int64_t ired_combine(int64_t x, int64_t y) {
  if constexpr (OP == kIRedMax) return x > y ? x : y;
  else if constexpr (OP == kIRedMin) return x < y ? x : y;
  else return (int64_t)((uint64_t)x + (uint64_t)y);
}
template <int OP> __device__ __forceinline__ int64_t iblock_reduce(int64_t v) {
  constexpr int kWaves = kRedBlock / kWave;
  __shared__ long long partial[kWaves];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = ired_combine<OP>(v, (int64_t)__shfl_xor((long long)v, off, kWave));
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) partial[wid] = v;
  __syncthreads();
  int64_t r = ired_init<OP>();
  if (wid == 0) {
    r = lane < kWaves ? (int64_t)partial[lane] : ired_init<OP>();
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) r = ired_combine<OP>(r, (int64_t)__shfl_xor((long long)r, off, kWave));
  }
  return r;  // valid in thread 0
}

template <int OP, bool NT>
__global__ __launch_bounds__(kRedBlock) void int_reduce_kernel(const int64_t* __restrict__ a, int64_t n, Split sp,
                                                               int64_t* __restrict__ partials,
                                                               unsigned* __restrict__ ticket,
                                                               int64_t* __restrict__ out) {
  constexpr int U = 8;
  const int64_t stride = (int64_t)gridDim.x * kRedBlock;
  const int64_t tid = (int64_t)blockIdx.x * kRedBlock + threadIdx.x;
  int64_t acc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) acc[u] = ired_init<OP>();
  if (tid < sp.head) acc[0] = a[tid];
  const I64Vec* av = reinterpret_cast<const I64Vec*>(a + sp.head);
  int64_t i = tid;
  for (; i + (U - 1) * stride < sp.nvec; i += U * stride) {
    I64Vec va[U];
#pragma unroll
    for (int u = 0; u < U; ++u) va[u] = ld16<NT>(av + i + u * stride);
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = ired_combine<OP>(acc[u], ired_combine<OP>(va[u].v[0], va[u].v[1]));
  }
  for (; i < sp.nvec; i += stride) {
    const I64Vec va = av[i];
    acc[0] = ired_combine<OP>(acc[0], ired_combine<OP>(va.v[0], va.v[1]));
  }
  for (int64_t k = sp.head + sp.nvec * 2 + tid; k < n; k += stride) acc[0] = ired_combine<OP>(acc[0], a[k]);
#pragma unroll
  for (int u = 1; u < U; ++u) acc[0] = ired_combine<OP>(acc[0], acc[u]);
  const int64_t mine = iblock_reduce<OP>(acc[0]);
  if (threadIdx.x == 0) publish(partials + blockIdx.x, mine);
  if (!take_last_ticket(ticket, gridDim.x)) return;
  const int count = (int)gridDim.x;
  int64_t r = ired_init<OP>();
  for (int j = threadIdx.x; j < count; j += kRedBlock) r = ired_combine<OP>(r, load_agent(partials + j));
  r = iblock_reduce<OP>(r);
  if (threadIdx.x == 0) {
    *out = r;
    rearm(ticket);
  }
}

// ---- casts ---------------------------------------------------------------------------
// float -> int64 truncates toward zero; NaN, +-inf and anything outside
// [-2^63, 2^63) give INT64_MIN (numpy's astype on x86-64: cvttsd2si's answer)
template <typename F> __device__ __forceinline__ int64_t float_to_i64(F x) {
  return (x >= F(-9223372036854775808.0) && x < F(9223372036854775808.0)) ? (int64_t)x : kI64Min;
}
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void int_cast_kernel(const TI* __restrict__ x, TO* __restrict__ y, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if constexpr (std::is_same<TI, uint8_t>::value) y[i] = x[i] != 0 ? 1 : 0;
    else if constexpr (std::is_same<TI, int64_t>::value) y[i] = (TO)x[i];  // round to nearest even
    else y[i] = float_to_i64<TI>(x[i]);
  }
}

// ---- draws -----------------------------------------------------------------------------
// Element i of a draw depends on (seed, offset, i) and the parameters alone.
// Every rejection loop is bounded by kMaxRintAttempts Philox calls; a lane that
// exhausts them stores its current candidate, clamped into the support.
constexpr uint32_t kMaxRintAttempts = 64;

// integers, span <= 2^32: counter (offset + q, tag, attempt) -> elements 4q .. 4q + 3,
// one word each.  Lemire's multiply-shift: m = w * s, accepted iff the low
// word >= 2^32 mod s; a rejected word is redrawn as the same word of the next attempt.
template <bool NT>
__global__ __launch_bounds__(256) void rint_small_kernel(int64_t* __restrict__ out, int64_t n, uint32_t k0, uint32_t k1,
                                                         uint64_t offset, int64_t low, uint64_t s, uint32_t thresh,
                                                         bool vec) {
  const int64_t quads = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += stride) {
    const uint64_t ctr = offset + (uint64_t)q;
    int64_t v[4];
    unsigned pending = 0xfu;
    for (uint32_t j = 0; j < kMaxRintAttempts && pending; ++j) {
      const uint4 r = Philox::run(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), kTagIntSmall, j), k0, k1);
      const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (!(pending & (1u << e))) continue;
        const uint64_t m = (uint64_t)w[e] * s;
        v[e] = (int64_t)((uint64_t)low + (m >> 32));
        if ((uint32_t)m >= thresh) pending &= ~(1u << e);
      }
    }
    const int64_t i = 4 * q;
    if (vec && i + 3 < n) {
      I64Vec lo2, hi2;
      lo2.v[0] = v[0], lo2.v[1] = v[1], hi2.v[0] = v[2], hi2.v[1] = v[3];
      st16<NT>(reinterpret_cast<I64Vec*>(out + i), lo2);
      st16<NT>(reinterpret_cast<I64Vec*>(out + i + 2), hi2);
    } else {
      for (int e = 0; e < 4 && i + e < n; ++e) out[i + e] = v[e];
    }
  }
}

// integers, span > 2^32: counter -> elements 2p, 2p + 1 from the 64-bit words
// w0 << 32 | w1 and w2 << 32 | w3; the 128-bit product's high half is the
// value, accepted iff its low half >= 2^64 mod s.
template <bool NT>
__global__ __launch_bounds__(256) void rint_large_kernel(int64_t* __restrict__ out, int64_t n, uint32_t k0, uint32_t k1,
                                                         uint64_t offset, int64_t low, uint64_t s, uint64_t thresh,
                                                         bool vec) {
  const int64_t pairs = (n + 1) / 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pairs; p += stride) {
    const uint64_t ctr = offset + (uint64_t)p;
    int64_t v[2];
    unsigned pending = 0x3u;
    for (uint32_t j = 0; j < kMaxRintAttempts && pending; ++j) {
      const uint4 r = Philox::run(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), kTagIntLarge, j), k0, k1);
      const uint64_t w[2] = {((uint64_t)r.x << 32) | r.y, ((uint64_t)r.z << 32) | r.w};
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (!(pending & (1u << e))) continue;
        v[e] = (int64_t)((uint64_t)low + __umul64hi(w[e], s));
        if (w[e] * s >= thresh) pending &= ~(1u << e);
      }
    }
    const int64_t i = 2 * p;
    if (vec && i + 1 < n) {
      I64Vec o;
      o.v[0] = v[0], o.v[1] = v[1];
      st16<NT>(reinterpret_cast<I64Vec*>(out + i), o);
    } else {
      out[i] = v[0];
      if (i + 1 < n) out[i + 1] = v[1];
    }
  }
}

// geometric: two elements per counter from open 53-bit uniforms, as kinds 0-7
// of bk_rand_dist: k = ceil(log1p(-u) / log1p(-p)), at least 1, at most INT64_MAX
__device__ __forceinline__ int64_t geometric_of(double u, double lp) {
  const double k = ceil(log1p(-u) / lp);
  if (!(k >= 1.0)) return 1;
  return k >= 9223372036854775808.0 ? kI64Max : (int64_t)k;
}
__global__ __launch_bounds__(256) void rint_geometric_kernel(int64_t* __restrict__ out, int64_t n, uint32_t k0,
                                                             uint32_t k1, uint64_t offset, double lp, bool one) {
  const int64_t pairs = (n + 1) / 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pairs; p += stride) {
    const uint64_t ctr = offset + (uint64_t)p;
    const uint4 r = Philox::run(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), kTagGeometric, 0u), k0, k1);
    const int64_t i = 2 * p;
    out[i] = one ? 1 : geometric_of(u53_open(r.x, r.y), lp);
    if (i + 1 < n) out[i + 1] = one ? 1 : geometric_of(u53_open(r.z, r.w), lp);
  }
}

// poisson and binomial: element i owns the substream (offset + i, tag, attempt).
// The constants are computed once on the host (bk_rand_int); the arithmetic
// below is written operation by operation as tests/int_ref.py's model has it
// (no contraction into fma: an accept decision must not depend on it).
struct PoissonParams {
  double lam, enlam;                              // the multiplication method (lam < 10)
  double loglam, b, a, log_invalpha, vr;          // PTRS (lam >= 10)
};
struct BinomialParams {
  double n, p, q;                                  // trials, p' = min(p, 1 - p), 1 - p'
  double qn, bound;                                // inversion (n p' < 10)
  double b, a, c, vr, alpha, m, h, lpq;            // BTRS: h = lgamma(m + 1) + lgamma(n - m + 1), lpq = log(p' / q)
  int64_t trials;
  bool flip, zero, inversion;                      // p > 0.5: return trials - k; n = 0 or p' = 0: k = 0
};

__device__ __forceinline__ int64_t poisson_draw(uint64_t ctr, uint32_t k0, uint32_t k1, const PoissonParams& P) {
#pragma clang fp contract(off)
  const uint32_t lo = (uint32_t)ctr, hi = (uint32_t)(ctr >> 32);
  if (P.lam == 0.0) return 0;
  if (P.lam < 10.0) {
    // numpy's multiplication method: the count of factors taken before the product falls to exp(-lam)
    int64_t x = 0;
    double prod = 1.0;
    for (uint32_t j = 0; j < kMaxRintAttempts; ++j) {
      const uint4 r = Philox::run(make_uint4(lo, hi, kTagPoisson, j), k0, k1);
      const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        prod = prod * u32_open(w[e]);
        if (prod <= P.enlam) return x;
        ++x;
      }
    }
    return x;
  }
  // Hoermann's PTRS (transformed rejection with squeeze), numpy's constants
  int64_t res = 0;
  for (uint32_t j = 0; j < kMaxRintAttempts; ++j) {
    const uint4 r = Philox::run(make_uint4(lo, hi, kTagPoisson, j), k0, k1);
    const double U = u53_open(r.x, r.y) - 0.5, V = u53_open(r.z, r.w);
    const double us = 0.5 - fabs(U);
    const double k = floor((2.0 * P.a / us + P.b) * U + P.lam + 0.43);
    res = k < 0.0 ? 0 : (int64_t)k;
    if (us >= 0.07 && V <= P.vr) return res;
    if (k < 0.0 || (us < 0.013 && V > us)) continue;
    if (log(V) + P.log_invalpha - log(P.a / (us * us) + P.b) <= -P.lam + k * P.loglam - lgamma(k + 1.0)) return res;
  }
  return res;
}

__device__ __forceinline__ int64_t binomial_draw(uint64_t ctr, uint32_t k0, uint32_t k1, const BinomialParams& B) {
#pragma clang fp contract(off)
  const uint32_t lo = (uint32_t)ctr, hi = (uint32_t)(ctr >> 32);
  int64_t res = 0;
  if (B.zero) {
    res = 0;
  } else if (B.inversion) {
    // numpy's inversion: walk the pmf from 0 with px <- (n - X + 1) p px / (X q)
    for (uint32_t j = 0; j < kMaxRintAttempts; ++j) {
      const uint4 r = Philox::run(make_uint4(lo, hi, kTagBinomial, j), k0, k1);
      double u = u53_open(r.x, r.y), px = B.qn, x = 0.0;
      bool restart = false;
      while (u > px) {
        x = x + 1.0;
        if (x > B.bound) {
          restart = true;
          break;
        }
        u = u - px;
        px = ((B.n - x + 1.0) * B.p * px) / (x * B.q);
      }
      res = (int64_t)(x > B.n ? B.n : x);
      if (!restart) break;
    }
  } else {
    // Hoermann's BTRS; the acceptance test is the exact log pmf ratio
    for (uint32_t j = 0; j < kMaxRintAttempts; ++j) {
      const uint4 r = Philox::run(make_uint4(lo, hi, kTagBinomial, j), k0, k1);
      const double U = u53_open(r.x, r.y) - 0.5, V = u53_open(r.z, r.w);
      const double us = 0.5 - fabs(U);
      const double k = floor((2.0 * B.a / us + B.b) * U + B.c);
      res = (int64_t)(k < 0.0 ? 0.0 : k > B.n ? B.n : k);
      if (us >= 0.07 && V <= B.vr) break;
      if (k < 0.0 || k > B.n) continue;
      if (log(V * B.alpha / (B.a / (us * us) + B.b)) <=
          B.h - lgamma(k + 1.0) - lgamma(B.n - k + 1.0) + (k - B.m) * B.lpq)
        break;
    }
  }
  return B.flip ? B.trials - res : res;
}

__global__ __launch_bounds__(256) void rint_poisson_kernel(int64_t* __restrict__ out, int64_t n, uint32_t k0,
                                                           uint32_t k1, uint64_t offset, PoissonParams P) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = poisson_draw(offset + (uint64_t)i, k0, k1, P);
}
__global__ __launch_bounds__(256) void rint_binomial_kernel(int64_t* __restrict__ out, int64_t n, uint32_t k0,
                                                            uint32_t k1, uint64_t offset, BinomialParams B) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = binomial_draw(offset + (uint64_t)i, k0, k1, B);
}

inline PoissonParams poisson_params(double lam) {
  PoissonParams P{};
  P.lam = lam;
  P.enlam = std::exp(-lam);
  if (lam >= 10.0) {
    const double slam = std::sqrt(lam);
    P.loglam = std::log(lam);
    P.b = 0.931 + 2.53 * slam;
    P.a = -0.059 + 0.02483 * P.b;
    P.log_invalpha = std::log(1.1239 + 1.1328 / (P.b - 3.4));
    P.vr = 0.9277 - 3.6224 / (P.b - 2.0);
  }
  return P;
}

inline BinomialParams binomial_params(int64_t trials, double p) {
  BinomialParams B{};
  B.trials = trials;
  B.flip = p > 0.5;
  B.n = (double)trials;
  B.p = B.flip ? 1.0 - p : p;
  B.q = 1.0 - B.p;
  B.zero = trials == 0 || B.p == 0.0;
  if (B.zero) return B;
  const double np = B.n * B.p;
  B.inversion = np < 10.0;
  if (B.inversion) {
    B.qn = std::exp(B.n * std::log1p(-B.p));
    B.bound = std::fmin(B.n, np + 10.0 * std::sqrt(np * B.q + 1.0));
  } else {
    const double spq = std::sqrt(np * B.q);
    B.b = 1.15 + 2.53 * spq;
    B.a = -0.0873 + 0.0248 * B.b + 0.01 * B.p;
    B.c = np + 0.5;
    B.vr = 0.92 - 4.2 / B.b;
    B.alpha = (2.83 + 5.1 / B.b) * spq;
    B.m = std::floor((B.n + 1.0) * B.p);
    B.h = std::lgamma(B.m + 1.0) + std::lgamma(B.n - B.m + 1.0);
    B.lpq = std::log(B.p / B.q);
  }
  return B;
}

// the parameter domains of bk_rand_int (beekern.h)
inline bool rand_int_params_ok(int kind, int64_t a, int64_t b, double p) {
  switch (kind) {
    case BK_RINT_INTEGERS: return b > a;
    case BK_RINT_POISSON: return p >= 0.0 && p <= 9007199254740992.0;
    case BK_RINT_BINOMIAL: return a >= 0 && a < (1ll << 53) && p >= 0.0 && p <= 1.0;
    case BK_RINT_GEOMETRIC: return p > 0.0 && p <= 1.0;
  }
  return false;
}

}  // namespace integer
}  // namespace bk

using namespace bk;
using namespace bk::integer;

// (contracts of the entry points: beekern.h)
BK_API int bk_int_binary(int op, int mode, const void* a, const void* b, int64_t scalar, void* y, int64_t n,
                         hipStream_t stream) {
  if (!a || !y || n < 0 || op < 0 || op >= kIBinCount || mode < 0 || mode > 2 || (mode == 0 && !b)) return kBadArgument;
  if (n == 0) return kOk;
  const Split sp = split_of(n, {a, mode == 0 ? b : nullptr, y});
  const unsigned g = stream_grid((n + 1) / 2, 256);
  return dispatch_op<kIBinCount>(op, [&](auto opc) {
    return dispatch_flag(mode == 0, [&](auto b_array) {
      return dispatch_flag(mode != 2, [&](auto a_left) {
        return dispatch_flag(stream_nt(n * 8), [&](auto nt) {
          constexpr bool BS = !decltype(b_array)::value, REV = !decltype(a_left)::value;
          if constexpr (BS || !REV)  // (no mode swaps two arrays)
            int_binary_kernel<decltype(opc)::value, BS, REV, decltype(nt)::value>
                <<<g, 256, 0, stream>>>((const int64_t*)a, (const int64_t*)b, scalar, (int64_t*)y, n, sp);
          return launch_status();
        });
      });
    });
  });
}

BK_API int bk_int_compare(int op, int mode, const void* a, const void* b, int64_t scalar, void* mask_out, int64_t n,
                          hipStream_t stream) {
  if (!a || !mask_out || n < 0 || op < 0 || op >= kICmpCount || mode < 0 || mode > 1 || (mode == 0 && !b))
    return kBadArgument;
  if (n == 0) return kOk;
  const Split sp = split_of(n, {a, mode == 0 ? b : nullptr});
  const bool y2 = (((uintptr_t)mask_out + (uintptr_t)sp.head) & 1) == 0;
  const unsigned g = stream_grid((n + 1) / 2, 256);
  return dispatch_op<kICmpCount>(op, [&](auto opc) {
    return dispatch_flag(mode == 0, [&](auto arrays) {
      return dispatch_flag(stream_nt(n * 8 * (mode == 0 ? 2 : 1)), [&](auto nt) {
        return dispatch_flag(y2, [&](auto y2c) {
          int_compare_kernel<decltype(opc)::value, !decltype(arrays)::value, decltype(nt)::value, decltype(y2c)::value>
              <<<g, 256, 0, stream>>>((const int64_t*)a, (const int64_t*)b, scalar, (uint8_t*)mask_out, n, sp);
          return launch_status();
        });
      });
    });
  });
}

BK_API int bk_int_reduce(int op, const void* a, int64_t n, void* workspace, void* out, hipStream_t stream) {
  if (!a || !workspace || !out || n < 0 || op < 0 || op >= kIRedCount) return kBadArgument;
  const Split sp = split_of(n, {a});
  const unsigned g = grid_blocks((n / 2 + kIntRedVecsPerLane - 1) / kIntRedVecsPerLane, kRedBlocks);
  int64_t* partials = (int64_t*)workspace;
  unsigned* ticket = reinterpret_cast<unsigned*>(partials + kRedMaxBlocks);
  return dispatch_op<kIRedCount>(op, [&](auto opc) {
    return dispatch_flag(stream_nt(n * 8), [&](auto nt) {
      int_reduce_kernel<decltype(opc)::value, decltype(nt)::value>
          <<<g, kRedBlock, 0, stream>>>((const int64_t*)a, n, sp, partials, ticket, (int64_t*)out);
      return launch_status();
    });
  });
}

BK_API int bk_int_cast(int src_dtype, int dst_dtype, const void* x, void* y, int64_t n, hipStream_t stream) {
  if (!x || !y || n < 0) return kBadArgument;
  const bool known = (src_dtype == kI64 && (dst_dtype == kF64 || dst_dtype == kF32)) ||
                     (dst_dtype == kI64 && (src_dtype == kF64 || src_dtype == kF32 || src_dtype == kBool));
  if (!known) return kBadArgument;
  if (n == 0) return kOk;
  const unsigned g = stream_grid(n, 256);
#define BK_ICAST(TI, TO) int_cast_kernel<TI, TO><<<g, 256, 0, stream>>>((const TI*)x, (TO*)y, n)
  if (src_dtype == kI64 && dst_dtype == kF64) BK_ICAST(int64_t, double);
  else if (src_dtype == kI64) BK_ICAST(int64_t, float);
  else if (src_dtype == kF64) BK_ICAST(double, int64_t);
  else if (src_dtype == kF32) BK_ICAST(float, int64_t);
  else BK_ICAST(uint8_t, int64_t);
#undef BK_ICAST
  return launch_status();
}

BK_API int bk_rand_int(int kind, void* out, int64_t n, uint64_t seed, uint64_t offset, int64_t a, int64_t b, double p,
                       hipStream_t stream) {
  if (kind < 0 || kind >= BK_RINT_COUNT || !out || n < 0 || !rand_int_params_ok(kind, a, b, p)) return kBadArgument;
  if (n == 0) return kOk;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  int64_t* o = (int64_t*)out;
  const bool vec = ((uintptr_t)out & 15) == 0;
  constexpr int kDrawBlocksPerCU = 256;  // as the uniform draws (bk_rand_uniform)
  switch (kind) {
    case BK_RINT_INTEGERS: {
      const uint64_t s = (uint64_t)b - (uint64_t)a;
      if (s <= (1ull << 32)) {
        const uint32_t thresh = (uint32_t)((1ull << 32) % s);
        const unsigned g = stream_grid((n + 3) / 4, 256, kDrawBlocksPerCU);
        if (stream_nt(n * 8)) rint_small_kernel<true><<<g, 256, 0, stream>>>(o, n, k0, k1, offset, a, s, thresh, vec);
        else rint_small_kernel<false><<<g, 256, 0, stream>>>(o, n, k0, k1, offset, a, s, thresh, vec);
      } else {
        const uint64_t thresh = (0ull - s) % s;  // 2^64 mod s
        const unsigned g = stream_grid((n + 1) / 2, 256, kDrawBlocksPerCU);
        if (stream_nt(n * 8)) rint_large_kernel<true><<<g, 256, 0, stream>>>(o, n, k0, k1, offset, a, s, thresh, vec);
        else rint_large_kernel<false><<<g, 256, 0, stream>>>(o, n, k0, k1, offset, a, s, thresh, vec);
      }
      break;
    }
    case BK_RINT_POISSON:
      rint_poisson_kernel<<<stream_grid(n, 256), 256, 0, stream>>>(o, n, k0, k1, offset, poisson_params(p));
      break;
    case BK_RINT_BINOMIAL:
      rint_binomial_kernel<<<stream_grid(n, 256), 256, 0, stream>>>(o, n, k0, k1, offset, binomial_params(a, p));
      break;
    default:  // BK_RINT_GEOMETRIC
      rint_geometric_kernel<<<stream_grid((n + 1) / 2, 256), 256, 0, stream>>>(o, n, k0, k1, offset, std::log1p(-p),
                                                                             p == 1.0);
      break;
  }
  return launch_status();
}
