// Counter-based Philox4x32-10 uniform generator: replaces numpy.random.rand
// in the benchmark payload (`examples/benchmark-numpy.py:20`, 1e8 f64).
//
// Element i of the stream depends only on (seed, i), never on the grid, so
// results are reproducible across launch shapes and GPU counts.  One Philox
// call yields 128 random bits = 2 f64 (numpy's 53-bit construction from two
// 32-bit draws, a>>5 and b>>6) or 4 f32 (24-bit), written with one 16-byte
// store per lane; the kernel is HBM-write bound (800 MB for 1e8 f64).
#include "bk_common.hpp"
#include "bk_philox.hpp"

namespace bk {

// out[i] = U[0,1) (f64), scaled to [lo, hi).  Each counter value -> 2 doubles.
// lo + span * u as one fma of the 53-bit integer (span * 2^-53 is exact: the
// same bits as rand_reduce_f64's fused draw, one f64 multiply fewer), and two
// counters per lane per iteration so two Philox chains overlap the stores.
template <bool NT>
__global__ __launch_bounds__(256) void philox_uniform_f64(double* __restrict__ out, int64_t n, uint32_t k0,
                                                          uint32_t k1, uint64_t offset, double lo, double span) {
  const int64_t pairs = (n + 1) / 2, full = n / 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const double s53 = span * (1.0 / 9007199254740992.0);
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; p + stride < full; p += 2 * stride) {
    const uint64_t c0 = offset + (uint64_t)p, c1 = c0 + (uint64_t)stride;
    const uint4 r0 = Philox::run(make_uint4((uint32_t)c0, (uint32_t)(c0 >> 32), kTagUniformF64, 0u), k0, k1);
    const uint4 r1 = Philox::run(make_uint4((uint32_t)c1, (uint32_t)(c1 >> 32), kTagUniformF64, 0u), k0, k1);
    st16<NT>(reinterpret_cast<double2*>(out + 2 * p),
             make_double2(fma(u53_int(r0.x, r0.y), s53, lo), fma(u53_int(r0.z, r0.w), s53, lo)));
    st16<NT>(reinterpret_cast<double2*>(out + 2 * (p + stride)),
             make_double2(fma(u53_int(r1.x, r1.y), s53, lo), fma(u53_int(r1.z, r1.w), s53, lo)));
  }
  for (; p < pairs; p += stride) {
    const uint64_t ctr = offset + (uint64_t)p;
    const uint4 r = Philox::run(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), kTagUniformF64, 0u), k0, k1);
    double2 v = make_double2(fma(u53_int(r.x, r.y), s53, lo), fma(u53_int(r.z, r.w), s53, lo));
    const int64_t i = 2 * p;
    if (i + 1 < n) {
      st16<NT>(reinterpret_cast<double2*>(out + i), v);  // 16-B store
    } else {
      out[i] = v.x;
    }
  }
}

// f32: each counter value -> 4 floats, one 16-B store.
template <bool NT>
__global__ __launch_bounds__(256) void philox_uniform_f32(float* __restrict__ out, int64_t n, uint32_t k0, uint32_t k1,
                                                          uint64_t offset, float lo, float span) {
  const int64_t quads = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += stride) {
    const uint64_t ctr = offset + (uint64_t)q;
    const uint4 r = Philox::run(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), kTagUniformF32, 0u), k0, k1);
    float4 v = make_float4(lo + span * u24(r.x), lo + span * u24(r.y), lo + span * u24(r.z), lo + span * u24(r.w));
    const int64_t i = 4 * q;
    if (i + 3 < n) {
      st16<NT>(reinterpret_cast<float4*>(out + i), v);
    } else {
      const float t[4] = {v.x, v.y, v.z, v.w};
      for (int j = 0; i + j < n; ++j) out[i + j] = t[j];
    }
  }
}

// bf16: the f32 stream's values rounded once to bf16 (RNE) -- bit-identical to
// drawing f32 and casting, without the f32 buffer and the cast pass.  Each
// lane handles two counters (8 values) for one 16-B store.
__global__ __launch_bounds__(256) void philox_uniform_bf16(uint16_t* __restrict__ out, int64_t n, uint32_t k0,
                                                           uint32_t k1, uint64_t offset, float lo, float span) {
  const int64_t octs = (n + 7) / 8;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < octs; o += stride) {
    uint16_t h[8];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const uint64_t ctr = offset + 2 * (uint64_t)o + half;
      const uint4 r = Philox::run(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), kTagUniformF32, 0u), k0, k1);
      h[4 * half + 0] = float_to_bf16_bits(lo + span * u24(r.x));
      h[4 * half + 1] = float_to_bf16_bits(lo + span * u24(r.y));
      h[4 * half + 2] = float_to_bf16_bits(lo + span * u24(r.z));
      h[4 * half + 3] = float_to_bf16_bits(lo + span * u24(r.w));
    }
    const int64_t i = 8 * o;
    if (i + 7 < n) {
      *reinterpret_cast<uint4*>(out + i) = make_uint4(h[0] | ((uint32_t)h[1] << 16), h[2] | ((uint32_t)h[3] << 16),
                                                      h[4] | ((uint32_t)h[5] << 16), h[6] | ((uint32_t)h[7] << 16));
    } else {
      for (int j = 0; i + j < n; ++j) out[i + j] = h[j];
    }
  }
}

// Standard normal via Box-Muller on the f32 / f64 streams (for randn).
__global__ __launch_bounds__(256) void philox_normal_f32(float* __restrict__ out, int64_t n, uint32_t k0, uint32_t k1,
                                                         uint64_t offset, float mean, float std) {
  const int64_t quads = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += stride) {
    const uint64_t ctr = offset + (uint64_t)q;
    const uint4 r = Philox::run(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), 0x6e6f726du, 0u), k0, k1);
    const float u1 = fmaxf(u24(r.x), 1e-12f), u2 = u24(r.y), u3 = fmaxf(u24(r.z), 1e-12f), u4 = u24(r.w);
    const float r1 = sqrtf(-2.f * __logf(u1)), r2 = sqrtf(-2.f * __logf(u3));
    float s1, c1, s2, c2;
    __sincosf(6.283185307f * u2, &s1, &c1);
    __sincosf(6.283185307f * u4, &s2, &c2);
    const float t[4] = {mean + std * r1 * c1, mean + std * r1 * s1, mean + std * r2 * c2, mean + std * r2 * s2};
    const int64_t i = 4 * q;
    if (i + 3 < n) {
      *reinterpret_cast<float4*>(out + i) = make_float4(t[0], t[1], t[2], t[3]);
    } else {
      for (int j = 0; i + j < n; ++j) out[i + j] = t[j];
    }
  }
}

__global__ __launch_bounds__(256) void philox_normal_f64(double* __restrict__ out, int64_t n, uint32_t k0, uint32_t k1,
                                                         uint64_t offset, double mean, double std) {
  const int64_t pairs = (n + 1) / 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pairs; p += stride) {
    const uint64_t ctr = offset + (uint64_t)p;
    const uint4 r = Philox::run(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), 0x6e6f726eu, 0u), k0, k1);
    const double u1 = fmax(u53(r.x, r.y), 1e-300), u2 = u53(r.z, r.w);
    const double rad = sqrt(-2.0 * log(u1));
    double s, c;
    sincos(6.283185307179586 * u2, &s, &c);
    const int64_t i = 2 * p;
    if (i + 1 < n) {
      *reinterpret_cast<double2*>(out + i) = make_double2(mean + std * rad * c, mean + std * rad * s);
    } else {
      out[i] = mean + std * rad * c;
    }
  }
}

// ---- bk_rand_dist: twelve continuous distributions ----------------------------------------
//
// Kinds 0-7 are one transform of one open-interval uniform, packed exactly as
// the uniform draws (a counter -> 2 f64 from 53-bit uniforms, or 4 f32 from
// 24-bit uniforms in f32 arithmetic), on tags of their own.  The library's
// accurate log / log1p / expm1 / tan / pow: the results are checked against
// their formulas (tests/dist_ref.py), not against a fast intrinsic's error.

__device__ __forceinline__ float m_log(float x) { return logf(x); }
__device__ __forceinline__ double m_log(double x) { return log(x); }
__device__ __forceinline__ float m_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double m_log1p(double x) { return log1p(x); }
__device__ __forceinline__ float m_expm1(float x) { return expm1f(x); }
__device__ __forceinline__ double m_expm1(double x) { return expm1(x); }
__device__ __forceinline__ float m_tan(float x) { return tanf(x); }
__device__ __forceinline__ double m_tan(double x) { return tan(x); }
__device__ __forceinline__ float m_pow(float x, float y) { return powf(x, y); }
__device__ __forceinline__ double m_pow(double x, double y) { return pow(x, y); }
__device__ __forceinline__ float m_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double m_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float m_abs(float x) { return fabsf(x); }
__device__ __forceinline__ double m_abs(double x) { return fabs(x); }
__device__ __forceinline__ float m_copysign(float x, float y) { return copysignf(x, y); }
__device__ __forceinline__ double m_copysign(double x, double y) { return copysign(x, y); }

// u in (0, 1), so E = -log1p(-u) is finite and positive and no value is inf or
// NaN.  numpy's formulas (legacy-distributions.c), with its 1 - U our u.
template <int KIND, typename T>
__device__ __forceinline__ T dist_transform(T u, T p0, T p1) {
  if constexpr (KIND == BK_DIST_LAPLACE) {
    return u >= T(0.5) ? p0 - p1 * m_log(T(2) - T(2) * u) : p0 + p1 * m_log(T(2) * u);
  } else if constexpr (KIND == BK_DIST_LOGISTIC) {
    return p0 + p1 * m_log(u / (T(1) - u));
  } else if constexpr (KIND == BK_DIST_CAUCHY) {
    // tan(pi (u - 1/2)), evaluated where its argument is exact: near the poles
    // as 1 / tan(pi (1/2 - |x|)), whose small argument is exact (u, 1/2 - |x|
    // are) -- tan of the rounded product pi x next to pi / 2 would lose every digit in f32
    const T x = u - T(0.5), ax = m_abs(x);
    const bool inner = ax <= T(0.25);
    const T t = m_tan(T(3.14159265358979323846) * (inner ? ax : T(0.5) - ax));
    return p0 + p1 * m_copysign(inner ? t : T(1) / t, x);
  } else {
    const T e = -m_log1p(-u);  // the standard exponential
    if constexpr (KIND == BK_DIST_EXPONENTIAL) return p0 * e;
    else if constexpr (KIND == BK_DIST_GUMBEL) return p0 - p1 * m_log(e);
    else if constexpr (KIND == BK_DIST_RAYLEIGH) return p0 * m_sqrt(T(2) * e);
    else if constexpr (KIND == BK_DIST_WEIBULL) return m_pow(e, T(1) / p0);
    else return m_expm1(e / p0);  // pareto (Lomax)
  }
}

template <int KIND, bool NT>
__global__ __launch_bounds__(256) void philox_dist_f64(double* __restrict__ out, int64_t n, uint32_t k0, uint32_t k1,
                                                       uint64_t offset, double p0, double p1) {
  const int64_t pairs = (n + 1) / 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pairs; p += stride) {
    const uint64_t ctr = offset + (uint64_t)p;
    const uint4 r = Philox::run(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), kTagDistF64, 0u), k0, k1);
    const double2 v = make_double2(dist_transform<KIND, double>(u53_open(r.x, r.y), p0, p1),
                                   dist_transform<KIND, double>(u53_open(r.z, r.w), p0, p1));
    const int64_t i = 2 * p;
    if (i + 1 < n) {
      st16<NT>(reinterpret_cast<double2*>(out + i), v);
    } else {
      out[i] = v.x;
    }
  }
}

template <int KIND, bool NT>
__global__ __launch_bounds__(256) void philox_dist_f32(float* __restrict__ out, int64_t n, uint32_t k0, uint32_t k1,
                                                       uint64_t offset, float p0, float p1) {
  const int64_t quads = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += stride) {
    const uint64_t ctr = offset + (uint64_t)q;
    const uint4 r = Philox::run(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), kTagDistF32, 0u), k0, k1);
    const float4 v = make_float4(
        dist_transform<KIND, float>(u24_open(r.x), p0, p1), dist_transform<KIND, float>(u24_open(r.y), p0, p1),
        dist_transform<KIND, float>(u24_open(r.z), p0, p1), dist_transform<KIND, float>(u24_open(r.w), p0, p1));
    const int64_t i = 4 * q;
    if (i + 3 < n) {
      st16<NT>(reinterpret_cast<float4*>(out + i), v);
    } else {
      const float t[4] = {v.x, v.y, v.z, v.w};
      for (int j = 0; i + j < n; ++j) out[i + j] = t[j];
    }
  }
}

// Lognormal: exp of the value philox_normal_* writes for the same (seed,
// offset, mean, sigma) -- the same tags, words and expressions (the f32 path
// keeps the fast log and sincos so the normal's bits agree), one exp and no
// second pass over the array.
template <bool NT>
__global__ __launch_bounds__(256) void philox_lognormal_f32(float* __restrict__ out, int64_t n, uint32_t k0,
                                                            uint32_t k1, uint64_t offset, float mean, float std) {
  const int64_t quads = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += stride) {
    const uint64_t ctr = offset + (uint64_t)q;
    const uint4 r = Philox::run(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), kTagNormalF32, 0u), k0, k1);
    const float u1 = fmaxf(u24(r.x), 1e-12f), u2 = u24(r.y), u3 = fmaxf(u24(r.z), 1e-12f), u4 = u24(r.w);
    const float r1 = sqrtf(-2.f * __logf(u1)), r2 = sqrtf(-2.f * __logf(u3));
    float s1, c1, s2, c2;
    __sincosf(6.283185307f * u2, &s1, &c1);
    __sincosf(6.283185307f * u4, &s2, &c2);
    const float t[4] = {expf(mean + std * r1 * c1), expf(mean + std * r1 * s1), expf(mean + std * r2 * c2),
                        expf(mean + std * r2 * s2)};
    const int64_t i = 4 * q;
    if (i + 3 < n) {
      st16<NT>(reinterpret_cast<float4*>(out + i), make_float4(t[0], t[1], t[2], t[3]));
    } else {
      for (int j = 0; i + j < n; ++j) out[i + j] = t[j];
    }
  }
}

template <bool NT>
__global__ __launch_bounds__(256) void philox_lognormal_f64(double* __restrict__ out, int64_t n, uint32_t k0,
                                                            uint32_t k1, uint64_t offset, double mean, double std) {
  const int64_t pairs = (n + 1) / 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pairs; p += stride) {
    const uint64_t ctr = offset + (uint64_t)p;
    const uint4 r = Philox::run(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), kTagNormalF64, 0u), k0, k1);
    const double u1 = fmax(u53(r.x, r.y), 1e-300), u2 = u53(r.z, r.w);
    const double rad = sqrt(-2.0 * log(u1));
    double s, c;
    sincos(6.283185307179586 * u2, &s, &c);
    const int64_t i = 2 * p;
    if (i + 1 < n) {
      st16<NT>(reinterpret_cast<double2*>(out + i), make_double2(exp(mean + std * rad * c), exp(mean + std * rad * s)));
    } else {
      out[i] = exp(mean + std * rad * c);
    }
  }
}

// ---- the rejection family: gamma, beta, student t -----------------------------------------
//
// Marsaglia & Tsang (2000) for shape >= 1: with d = shape - 1/3 and
// c = 1 / sqrt(9 d), draw a normal x and a uniform u until v = (1 + c x)^3 > 0
// and u < 1 - 0.0331 x^4 (the squeeze) or log u < x^2 / 2 + d (1 - v + log v);
// the value is d v.  A shape below 1 draws at shape + 1 and multiplies by
// U^(1 / shape).
//
// Element i owns a substream: the counter (offset + i, tag, attempt j).  One
// attempt is one Philox call: words 0, 1 -> the open 53-bit uniform of the
// Box-Muller radius, word 2 -> its angle ((w + 1/2) 2^-32 turns, the cosine
// branch only), word 3 -> the acceptance uniform (w + 1/2) 2^-32.  So a value
// depends on (seed, offset + i) alone, never on the grid or on its neighbours,
// and a draw advances the counter by one per element.  The boost uniform is
// words 0, 1 of attempt 0 on the tag kTagBoost above the gamma's.
//
// All of it in f64, whatever the output: the f32 result is the f64 value
// rounded once, so an accept decision never depends on the dtype.
//
// One element per lane.  A wave runs as long as its slowest lane -- with a
// rejection rate below 5 % (shape >= 1) that is 2 attempts for most waves, 3
// for a few -- and the two logs of the full test run whenever one of the 64
// lanes misses the squeeze, which is nearly always: per element about two
// attempts' worth of f64 log / cos / log / log, which is what bounds the
// kernel, not the store.  The loop is bounded: after kMaxAttempts rejections
// (probability below 0.05^64) the lane stores d, the value at x = 0.
constexpr uint32_t kMaxAttempts = 64;

struct GammaShape {
  double d, c;    // of the shape drawn at (shape + 1 below 1)
  double boost;   // 1 / shape for a shape below 1, else 0: no boost
};

__device__ __forceinline__ double attempt_normal(const uint4 r) {
  return sqrt(-2.0 * log(u53_open(r.x, r.y))) * cospi(2.0 * u32_open(r.z));
}

__device__ __forceinline__ double gamma_draw(uint64_t ctr, uint32_t tag, uint32_t k0, uint32_t k1, const GammaShape g) {
  const uint32_t lo = (uint32_t)ctr, hi = (uint32_t)(ctr >> 32);
  double res = g.d;
  for (uint32_t j = 0; j < kMaxAttempts; ++j) {
    const uint4 r = Philox::run(make_uint4(lo, hi, tag, j), k0, k1);
    const double x = attempt_normal(r), u = u32_open(r.w);
    const double t = 1.0 + g.c * x, v = t * t * t, x2 = x * x;
    if (t > 0.0 && (u < 1.0 - 0.0331 * (x2 * x2) || log(u) < 0.5 * x2 + g.d * (1.0 - v + log(v)))) {
      res = g.d * v;
      break;
    }
  }
  if (g.boost != 0.0) {  // (uniform across the launch)
    const uint4 r = Philox::run(make_uint4(lo, hi, tag + kTagBoost, 0u), k0, k1);
    res *= exp(log(u53_open(r.x, r.y)) * g.boost);
  }
  return res;
}

// the log of the same draw, for the ratio of two draws that both underflowed
__device__ __forceinline__ double gamma_draw_log(uint64_t ctr, uint32_t tag, uint32_t k0, uint32_t k1, GammaShape g) {
  const double boost = g.boost;
  g.boost = 0.0;
  double l = log(gamma_draw(ctr, tag, k0, k1, g));
  if (boost != 0.0) {
    const uint4 r = Philox::run(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), tag + kTagBoost, 0u), k0, k1);
    l += log(u53_open(r.x, r.y)) * boost;
  }
  return l;
}

template <int KIND, typename T>
__global__ __launch_bounds__(256) void philox_reject(T* __restrict__ out, int64_t n, uint32_t k0, uint32_t k1,
                                                     uint64_t offset, GammaShape ga, GammaShape gb, double scale) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t ctr = offset + (uint64_t)i;
    double v;
    if constexpr (KIND == BK_DIST_GAMMA) {
      v = gamma_draw(ctr, kTagGammaX, k0, k1, ga) * scale;
    } else if constexpr (KIND == BK_DIST_BETA) {
      const double x = gamma_draw(ctr, kTagGammaX, k0, k1, ga), y = gamma_draw(ctr, kTagGammaY, k0, k1, gb);
      if (x + y > 0.0) {
        v = x / (x + y);
      } else {
        // both boosts underflowed (shapes far below 1): the same ratio from the logs
        v = 1.0 / (1.0 + exp(gamma_draw_log(ctr, kTagGammaY, k0, k1, gb) - gamma_draw_log(ctr, kTagGammaX, k0, k1, ga)));
      }
    } else {  // student t: N sqrt(df / (2 G)), G ~ gamma(df / 2); scale carries df
      const uint4 r = Philox::run(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), kTagStudentN, 0u), k0, k1);
      // (a G that underflowed to 0 is held at the smallest normal: a finite value)
      const double g = fmax(gamma_draw(ctr, kTagGammaX, k0, k1, ga), 2.2250738585072014e-308);
      v = attempt_normal(r) * sqrt(scale / (2.0 * g));
    }
    out[i] = (T)v;
  }
}

inline GammaShape gamma_shape(double shape) {
  const double s = shape < 1.0 ? shape + 1.0 : shape;
  const double d = s - 1.0 / 3.0;
  return GammaShape{d, 1.0 / sqrt(9.0 * d), shape < 1.0 ? 1.0 / shape : 0.0};
}

// finite, and inside the kind's domain: scale and sigma >= 0; shape, a, b and df > 0
inline bool dist_params_ok(int kind, double p0, double p1) {
  if (!std::isfinite(p0) || !std::isfinite(p1)) return false;
  switch (kind) {
    case BK_DIST_EXPONENTIAL: case BK_DIST_RAYLEIGH: return p0 >= 0.0;
    case BK_DIST_LAPLACE: case BK_DIST_LOGISTIC: case BK_DIST_GUMBEL: case BK_DIST_CAUCHY: case BK_DIST_LOGNORMAL:
      return p1 >= 0.0;
    case BK_DIST_WEIBULL: case BK_DIST_PARETO: case BK_DIST_STUDENT_T: return p0 > 0.0;
    case BK_DIST_GAMMA: return p0 > 0.0 && p1 >= 0.0;
    case BK_DIST_BETA: return p0 > 0.0 && p1 > 0.0;
  }
  return false;
}

template <int KIND>
void launch_dist(void* out, int64_t n, int dtype, uint32_t k0, uint32_t k1, uint64_t offset, double p0, double p1,
                 hipStream_t stream) {
  constexpr int kDrawBlocksPerCU = 256;  // as the uniform draws (bk_rand_uniform)
  if (dtype == kF64) {
    const unsigned g = stream_grid((n + 1) / 2, 256, kDrawBlocksPerCU);
    if (stream_nt(n * 8)) philox_dist_f64<KIND, true><<<g, 256, 0, stream>>>((double*)out, n, k0, k1, offset, p0, p1);
    else philox_dist_f64<KIND, false><<<g, 256, 0, stream>>>((double*)out, n, k0, k1, offset, p0, p1);
  } else {
    const unsigned g = stream_grid((n + 3) / 4, 256, kDrawBlocksPerCU);
    if (stream_nt(n * 4))
      philox_dist_f32<KIND, true><<<g, 256, 0, stream>>>((float*)out, n, k0, k1, offset, (float)p0, (float)p1);
    else
      philox_dist_f32<KIND, false><<<g, 256, 0, stream>>>((float*)out, n, k0, k1, offset, (float)p0, (float)p1);
  }
}

template <int KIND>
void launch_reject(void* out, int64_t n, int dtype, uint32_t k0, uint32_t k1, uint64_t offset, GammaShape ga,
                   GammaShape gb, double scale, hipStream_t stream) {
  const unsigned g = stream_grid(n, 256);
  if (dtype == kF64) philox_reject<KIND, double><<<g, 256, 0, stream>>>((double*)out, n, k0, k1, offset, ga, gb, scale);
  else philox_reject<KIND, float><<<g, 256, 0, stream>>>((float*)out, n, k0, k1, offset, ga, gb, scale);
}

}  // namespace bk

using namespace bk;

// (contracts of the entry points: beekern.h)
BK_API int bk_rand_uniform(void* out, int64_t n, int dtype, uint64_t seed, uint64_t offset, double lo, double hi,
                           hipStream_t stream) {
  if (!out || n < 0) return kBadArgument;
  if (n == 0) return kOk;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  // the f64 / f32 draws take a 4x larger grid cap than the elementwise
  // kernels: 1e8 f64 (800 MB), rocprofv3 mean / min: 64 blocks/CU 146 / 139
  // us, 128: 133 / 118, 256: 133 / 121, 512: 130 / 115
  // (profiles/archive/r3_philox_grid_sweep.log)
  constexpr int kDrawBlocksPerCU = 256;
  if (dtype == kF64) {
    const int64_t pairs = (n + 1) / 2;
    const unsigned g = stream_grid(pairs, 256, kDrawBlocksPerCU);
    if (stream_nt(n * 8)) philox_uniform_f64<true><<<g, 256, 0, stream>>>((double*)out, n, k0, k1, offset, lo, hi - lo);
    else philox_uniform_f64<false><<<g, 256, 0, stream>>>((double*)out, n, k0, k1, offset, lo, hi - lo);
  } else if (dtype == kBF16) {
    const int64_t octs = (n + 7) / 8;
    philox_uniform_bf16<<<stream_grid(octs, 256), 256, 0, stream>>>((uint16_t*)out, n, k0, k1, offset, (float)lo,
                                                                     (float)(hi - lo));
  } else if (dtype == kF32) {
    const int64_t quads = (n + 3) / 4;
    const unsigned g = stream_grid(quads, 256, kDrawBlocksPerCU);
    if (stream_nt(n * 4))
      philox_uniform_f32<true><<<g, 256, 0, stream>>>((float*)out, n, k0, k1, offset, (float)lo, (float)(hi - lo));
    else
      philox_uniform_f32<false><<<g, 256, 0, stream>>>((float*)out, n, k0, k1, offset, (float)lo, (float)(hi - lo));
  } else {
    return kBadArgument;
  }
  return launch_status();
}

BK_API int bk_rand_normal(void* out, int64_t n, int dtype, uint64_t seed, uint64_t offset, double mean, double std,
                          hipStream_t stream) {
  if (!out || n < 0) return kBadArgument;
  if (n == 0) return kOk;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  if (dtype == kF64) {
    philox_normal_f64<<<stream_grid((n + 1) / 2, 256), 256, 0, stream>>>((double*)out, n, k0, k1, offset, mean, std);
  } else if (dtype == kF32) {
    philox_normal_f32<<<stream_grid((n + 3) / 4, 256), 256, 0, stream>>>((float*)out, n, k0, k1, offset, (float)mean,
                                                                         (float)std);
  } else {
    return kBadArgument;
  }
  return launch_status();
}

BK_API int bk_rand_dist(int kind, void* out, int64_t n, int dtype, uint64_t seed, uint64_t offset, double p0, double p1,
                        hipStream_t stream) {
  if (kind < 0 || kind >= BK_DIST_COUNT || (dtype != kF64 && dtype != kF32) || !out || n < 0 ||
      !dist_params_ok(kind, p0, p1))
    return kBadArgument;
  if (n == 0) return kOk;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  switch (kind) {
    case BK_DIST_EXPONENTIAL: launch_dist<BK_DIST_EXPONENTIAL>(out, n, dtype, k0, k1, offset, p0, p1, stream); break;
    case BK_DIST_LAPLACE: launch_dist<BK_DIST_LAPLACE>(out, n, dtype, k0, k1, offset, p0, p1, stream); break;
    case BK_DIST_LOGISTIC: launch_dist<BK_DIST_LOGISTIC>(out, n, dtype, k0, k1, offset, p0, p1, stream); break;
    case BK_DIST_GUMBEL: launch_dist<BK_DIST_GUMBEL>(out, n, dtype, k0, k1, offset, p0, p1, stream); break;
    case BK_DIST_RAYLEIGH: launch_dist<BK_DIST_RAYLEIGH>(out, n, dtype, k0, k1, offset, p0, p1, stream); break;
    case BK_DIST_WEIBULL: launch_dist<BK_DIST_WEIBULL>(out, n, dtype, k0, k1, offset, p0, p1, stream); break;
    case BK_DIST_PARETO: launch_dist<BK_DIST_PARETO>(out, n, dtype, k0, k1, offset, p0, p1, stream); break;
    case BK_DIST_CAUCHY: launch_dist<BK_DIST_CAUCHY>(out, n, dtype, k0, k1, offset, p0, p1, stream); break;
    case BK_DIST_LOGNORMAL:
      if (dtype == kF64) {
        const unsigned g = stream_grid((n + 1) / 2, 256);
        if (stream_nt(n * 8)) philox_lognormal_f64<true><<<g, 256, 0, stream>>>((double*)out, n, k0, k1, offset, p0, p1);
        else philox_lognormal_f64<false><<<g, 256, 0, stream>>>((double*)out, n, k0, k1, offset, p0, p1);
      } else {
        const unsigned g = stream_grid((n + 3) / 4, 256);
        if (stream_nt(n * 4))
          philox_lognormal_f32<true><<<g, 256, 0, stream>>>((float*)out, n, k0, k1, offset, (float)p0, (float)p1);
        else
          philox_lognormal_f32<false><<<g, 256, 0, stream>>>((float*)out, n, k0, k1, offset, (float)p0, (float)p1);
      }
      break;
    case BK_DIST_GAMMA:
      launch_reject<BK_DIST_GAMMA>(out, n, dtype, k0, k1, offset, gamma_shape(p0), gamma_shape(1.0), p1, stream);
      break;
    case BK_DIST_BETA:
      launch_reject<BK_DIST_BETA>(out, n, dtype, k0, k1, offset, gamma_shape(p0), gamma_shape(p1), 1.0, stream);
      break;
    default:  // BK_DIST_STUDENT_T: the gamma of shape df / 2; `scale` carries df
      launch_reject<BK_DIST_STUDENT_T>(out, n, dtype, k0, k1, offset, gamma_shape(0.5 * p0), gamma_shape(1.0), p0, stream);
      break;
  }
  return launch_status();
}
