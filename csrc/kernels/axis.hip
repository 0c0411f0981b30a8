// 2-D arrays: a matrix combined with a vector along one axis (numpy's
// broadcasting of `X - X.mean(axis=0)`, `x / s.sum(axis=1, keepdims=True)`),
// and the per-column / per-row max, min, variance and standard deviation.
// f32 and f64 only.
//
// bk_broadcast streams the matrix once: every lane moves 16 bytes per access
// where the rows are 16-byte aligned (one element otherwise), four accesses
// in flight, non-temporal past the Infinity Cache.  A block of 256 lanes is a
// tile of CW column lanes x 256 / CW row lanes, CW the power of two that
// covers the row (at most 256): a 10^7 x 8 table fills its waves as a
// 10^4 x 10^4 one does, and row and column come from the grid and two loops,
// never from a division.  The vector's element is read once per lane and
// column tile (kind 0) or once per lane and row (kind 1).
//
// bk_axis_stat follows bk_reduce_axis (reduce.hip launch_axis): per row, a
// group of lanes owns the row (both variance passes in one kernel, the second
// re-reading the row from cache); per column, strips x row chunks publish f64
// partials and the block that takes a strip's last ticket folds them in chunk
// order, so results are the same bits run to run.  max / min return NaN for a
// line that holds one, as numpy.  The variance is numpy's two passes in f64:
// the mean of each line, kept in f64 (registers, or the workspace between the
// two launches of the column form), then the squared deviations from it.
#include <cmath>

#include "bk_binary_op.hpp"
#include "bk_common.hpp"
#include "bk_ticket.hpp"

namespace bk {
namespace axis {

template <typename T, int VEC> struct alignas(VEC * sizeof(T)) Pack { T v[VEC]; };

template <bool NT, typename P>
__device__ __forceinline__ P ldp(const P* p) {
  if constexpr (sizeof(P) == 16) return ld16<NT>(p);
  else return *p;
}
template <bool NT, typename P>
__device__ __forceinline__ void stp(P* p, const P& v) {
  if constexpr (sizeof(P) == 16) st16<NT>(p, v);
  else *p = v;
}

inline int log2_ceil(int64_t n, int cap_log) {
  int lg = 0;
  while (lg < cap_log && ((int64_t)1 << lg) < n) ++lg;
  return lg;
}

// ---- bk_broadcast ----------------------------------------------------------------
constexpr int kBcBlock = 256;

// y[r][c] = a[r][c] OP v[c] (KIND 0) or a[r][c] OP v[r] (KIND 1); SWAP: v OP a.
// `cvecs` row pieces of VEC elements; lg = log2 of the tile's column lanes.
// a and y may be the same matrix: a lane writes only what it has read.
template <typename T, int OP, int KIND, bool SWAP, int VEC, bool NT>
__global__ __launch_bounds__(kBcBlock) void broadcast_kernel(const T* a, const T* __restrict__ v, T* y, int64_t rows,
                                                            int64_t cvecs, int64_t lda, int64_t ldy, int lg) {
  using P = Pack<T, VEC>;
  constexpr int U = kStreamUnroll;
  const int cw = 1 << lg, rl_n = kBcBlock >> lg;
  const int cl = threadIdx.x & (cw - 1), rl = threadIdx.x >> lg;
  const int64_t cstep = (int64_t)gridDim.x * cw;
  const int64_t rstep = (int64_t)gridDim.y * U * rl_n;
  const int64_t cfirst = (int64_t)blockIdx.x * cw + cl;
  const int64_t rfirst = (int64_t)blockIdx.y * U * rl_n + rl;
  auto apply = [](P& x, const P& w) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) x.v[j] = SWAP ? binary<OP>(w.v[j], x.v[j]) : binary<OP>(x.v[j], w.v[j]);
  };
  // U rows of one column piece: loads, then the arithmetic, then the stores
  auto rows_of = [&](int64_t r0, int64_t cv, const P (&w)[U]) {
    P x[U];
    if (r0 + (int64_t)(U - 1) * rl_n < rows) {
#pragma unroll
      for (int u = 0; u < U; ++u)
        x[u] = ldp<NT>(reinterpret_cast<const P*>(a + (r0 + (int64_t)u * rl_n) * lda) + cv);
#pragma unroll
      for (int u = 0; u < U; ++u) apply(x[u], w[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) stp<NT>(reinterpret_cast<P*>(y + (r0 + (int64_t)u * rl_n) * ldy) + cv, x[u]);
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t r = r0 + (int64_t)u * rl_n;
        if (r < rows) {
          P t = ldp<NT>(reinterpret_cast<const P*>(a + r * lda) + cv);
          apply(t, w[u]);
          stp<NT>(reinterpret_cast<P*>(y + r * ldy) + cv, t);
        }
      }
    }
  };
  if constexpr (KIND == 0) {
    for (int64_t cv = cfirst; cv < cvecs; cv += cstep) {
      P w[U];
      w[0] = reinterpret_cast<const P*>(v)[cv];
#pragma unroll
      for (int u = 1; u < U; ++u) w[u] = w[0];
      for (int64_t r0 = rfirst; r0 < rows; r0 += rstep) rows_of(r0, cv, w);
    }
  } else {
    for (int64_t r0 = rfirst; r0 < rows; r0 += rstep) {
      P w[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t r = r0 + (int64_t)u * rl_n;
        const T s = r < rows ? v[r] : T(0);
#pragma unroll
        for (int j = 0; j < VEC; ++j) w[u].v[j] = s;
      }
      for (int64_t cv = cfirst; cv < cvecs; cv += cstep) rows_of(r0, cv, w);
    }
  }
}

template <typename T, int OP, int KIND, bool SWAP>
int launch_broadcast(const T* a, const T* v, T* y, int64_t rows, int64_t cols, int64_t lda, int64_t ldy, hipStream_t s) {
  constexpr int N = 16 / sizeof(T);
  const bool vec = cols % N == 0 && lda % N == 0 && ldy % N == 0 && (((uintptr_t)a | (uintptr_t)y) & 15) == 0 &&
                   (KIND == 1 || ((uintptr_t)v & 15) == 0);
  const int64_t cvecs = vec ? cols / N : cols;
  const int lg = log2_ceil(cvecs, 8);
  const int64_t cw = (int64_t)1 << lg, rl_n = kBcBlock >> lg;
  const int64_t cap = (int64_t)kNumCU * kStreamBlocksPerCU;
  int64_t gc = (cvecs + cw - 1) / cw;
  if (gc > cap) gc = cap;
  int64_t gr = (rows + kStreamUnroll * rl_n - 1) / (kStreamUnroll * rl_n);
  if (gr > cap / gc) gr = cap / gc > 0 ? cap / gc : 1;
  const dim3 grid((unsigned)gc, (unsigned)gr);
  if (vec)
    return dispatch_flag(stream_nt(rows * cols * (int64_t)sizeof(T)), [&](auto nt) {
      broadcast_kernel<T, OP, KIND, SWAP, N, decltype(nt)::value>
          <<<grid, kBcBlock, 0, s>>>(a, v, y, rows, cvecs, lda, ldy, lg);
      return launch_status();
    });
  broadcast_kernel<T, OP, KIND, SWAP, 1, false><<<grid, kBcBlock, 0, s>>>(a, v, y, rows, cvecs, lda, ldy, lg);
  return launch_status();
}

// bytes spanned by a rows x cols matrix of row stride ld; false if that wraps
inline bool span_bytes(int64_t rows, int64_t cols, int64_t ld, int64_t esize, uint64_t* out) {
  uint64_t e;
  if (__builtin_mul_overflow((uint64_t)(rows - 1), (uint64_t)ld, &e) || __builtin_add_overflow(e, (uint64_t)cols, &e))
    return false;
  return !__builtin_mul_overflow(e, (uint64_t)esize, out);
}
inline bool overlap(const void* p, uint64_t np, const void* q, uint64_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + nq && b < a + np;
}

// ---- bk_axis_stat ----------------------------------------------------------------
enum StatOp : int { kStatMax = 0, kStatMin, kStatVar, kStatStd, kStatCount };
// what a kernel accumulates: max, min, a sum (the mean pass), squared deviations
enum Mode : int { kMax = 0, kMin, kSum, kSqDev };

// The workspace: partials (chunks x columns, kAxisWsDoubles), the column means
// between the two launches of a column variance (as many), one ticket per
// column block (kAxisTickets) -- the sizes of reduce.hip's axis workspace
// (bk_ticket.hpp).

template <int MODE> __device__ __forceinline__ double init() {
  if constexpr (MODE == kMax) return -INFINITY;
  else if constexpr (MODE == kMin) return INFINITY;
  else return 0.0;
}
// max / min keep a NaN from either side (fmax / fmin would drop it)
template <int MODE> __device__ __forceinline__ double comb(double a, double b) {
  if constexpr (MODE == kMax) return (a > b || a != a) ? a : b;
  else if constexpr (MODE == kMin) return (a < b || a != a) ? a : b;
  else return a + b;
}
template <int MODE> __device__ __forceinline__ double take(double acc, double x, double mean) {
  if constexpr (MODE == kSqDev) {
    const double d = x - mean;
    return acc + d * d;
  } else {
    return comb<MODE>(acc, x);
  }
}
// a folded line's result: the mean pass stores f64 means, the rest the input dtype
template <int MODE, typename T>
__device__ __forceinline__ void finish_line(void* out, int64_t i, double v, double divisor, bool root) {
  if constexpr (MODE == kSum) {
    reinterpret_cast<double*>(out)[i] = v / divisor;
  } else if constexpr (MODE == kSqDev) {
    const double var = v / divisor;
    reinterpret_cast<T*>(out)[i] = (T)(root ? sqrt(var) : var);
  } else {
    reinterpret_cast<T*>(out)[i] = (T)v;
  }
}

// the chunk partials of `col` in a fixed order: four chains, loads in flight together
template <int MODE>
__device__ __forceinline__ double fold_chunks(const double* part, int chunks, int64_t cols, int64_t col) {
  double a[4] = {init<MODE>(), init<MODE>(), init<MODE>(), init<MODE>()};
  int c = 0;
  for (; c + 3 < chunks; c += 4) {
    double t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] = load_agent(part + (int64_t)(c + q) * cols + col);
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = comb<MODE>(a[q], t[q]);
  }
  for (; c < chunks; ++c) a[c & 3] = comb<MODE>(a[c & 3], load_agent(part + (int64_t)c * cols + col));
  return comb<MODE>(comb<MODE>(a[0], a[1]), comb<MODE>(a[2], a[3]));
}

// per column, one element per lane: a block owns 256 columns of one row chunk
template <typename T, int MODE>
__global__ __launch_bounds__(256) void col_stat(const T* __restrict__ x, int64_t rows, int64_t cols, int64_t ld,
                                                int64_t rows_per_chunk, double* __restrict__ part,
                                                unsigned* __restrict__ tickets, const double* __restrict__ means,
                                                void* __restrict__ out, double divisor, bool root) {
  const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (col < cols) {
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
    const int64_t r1 = r0 + rows_per_chunk < rows ? r0 + rows_per_chunk : rows;
    const double m = MODE == kSqDev ? means[col] : 0.0;
    double a[4] = {init<MODE>(), init<MODE>(), init<MODE>(), init<MODE>()};
    int64_t r = r0;
    for (; r + 3 < r1; r += 4) {
      T t[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] = x[(r + q) * ld + col];
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] = take<MODE>(a[q], (double)t[q], m);
    }
    for (; r < r1; ++r) a[0] = take<MODE>(a[0], (double)x[r * ld + col], m);
    publish(part + (int64_t)blockIdx.y * cols + col, comb<MODE>(comb<MODE>(a[0], a[1]), comb<MODE>(a[2], a[3])));
  }
  if (!take_last_ticket(tickets + blockIdx.x, gridDim.y)) return;
  if (col < cols) finish_line<MODE, T>(out, col, fold_chunks<MODE>(part, (int)gridDim.y, cols, col), divisor, root);
  if (threadIdx.x == 0) rearm(tickets + blockIdx.x);
}

// per column, 16-B vectors: the tile of reduce.hip's colsum_tile_v -- 16 waves
// own a strip of 2^lgc * V columns of one row chunk (16 column lanes, or as
// many as a narrower table has: the other lanes of the wave take more rows,
// so an 8-column table still uses every lane), a wave covers 64 >> lgc rows x
// the strip per step, up to four steps' loads in flight per lane
template <typename T, int MODE>
__global__ __launch_bounds__(kColWaves * 64) void col_stat_v(const T* __restrict__ x, int64_t rows, int64_t cols,
                                                            int64_t ld, int64_t rows_per_chunk,
                                                            double* __restrict__ part, unsigned* __restrict__ tickets,
                                                            const double* __restrict__ means, void* __restrict__ out,
                                                            double divisor, bool root, int lgc) {
  constexpr int V = 16 / sizeof(T);
  __shared__ double sacc[kColWaves][16 * V];
  const int W = V << lgc;  // strip width (columns)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cl = lane & ((1 << lgc) - 1), rl = lane >> lgc;  // column lane, row lane
  const int wave_rows = 64 >> lgc;
  const int64_t col0 = (int64_t)blockIdx.x * W + cl * V;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
  const int64_t r1 = r0 + rows_per_chunk < rows ? r0 + rows_per_chunk : rows;
  const int kStep = kColWaves * wave_rows;  // rows per block step
  double acc[V], m[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    acc[j] = init<MODE>();
    m[j] = 0.0;
  }
  if (col0 < cols) {  // (cols is a multiple of V: a lane's vector is inside or outside as a whole)
    if constexpr (MODE == kSqDev) {
#pragma unroll
      for (int j = 0; j < V; ++j) m[j] = means[col0 + j];
    }
    int64_t r = r0 + wave * wave_rows + rl;
    for (; r + 3 * kStep < r1; r += 4 * kStep) {
      V16<T> t[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] = *reinterpret_cast<const V16<T>*>(x + (r + (int64_t)q * kStep) * ld + col0);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = take<MODE>(acc[j], (double)t[q].v[j], m[j]);
    }
    for (; r < r1; r += kStep) {
      const V16<T> t = *reinterpret_cast<const V16<T>*>(x + r * ld + col0);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = take<MODE>(acc[j], (double)t.v[j], m[j]);
    }
  }
  // the row lanes of each column lane, the same order in every lane
  for (int off = 1 << lgc; off < 64; off <<= 1)
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = comb<MODE>(acc[j], __shfl_xor(acc[j], off, 64));
  if (rl == 0) {
#pragma unroll
    for (int j = 0; j < V; ++j) sacc[wave][cl * V + j] = acc[j];
  }
  __syncthreads();
  const int64_t col = (int64_t)blockIdx.x * W + threadIdx.x;
  if (threadIdx.x < W) {
    double s = sacc[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kColWaves; ++w) s = comb<MODE>(s, sacc[w][threadIdx.x]);
    if (col < cols) publish(part + (int64_t)blockIdx.y * cols + col, s);
  }
  if (!take_last_ticket(tickets + blockIdx.x, gridDim.y)) return;
  if (threadIdx.x < W && col < cols)
    finish_line<MODE, T>(out, col, fold_chunks<MODE>(part, (int)gridDim.y, cols, col), divisor, root);
  if (threadIdx.x == 0) rearm(tickets + blockIdx.x);
}

// per row: 2^lg lanes own a row (a whole wave for rows of 64 pieces or more,
// fewer for narrow tables, so a 10^7 x 8 table keeps every lane busy), each
// with four pieces of VEC elements in flight.  The lanes of a row fold with an
// xor butterfly, which leaves the same bits in all of them: the variance's
// mean stays in f64 registers for the second pass over the row.
template <typename T, int OP, int VEC>
__global__ __launch_bounds__(256) void row_stat(const T* __restrict__ x, int64_t rows, int64_t cvecs, int64_t ld,
                                                T* __restrict__ out, double n, double divisor, int lg) {
  using P = Pack<T, VEC>;
  constexpr int MODE = OP == kStatMax ? kMax : OP == kStatMin ? kMin : kSum;
  const int lanes = 1 << lg;
  const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> lg;
  if (row >= rows) return;  // (the lanes of a row leave together)
  const int l = threadIdx.x & (lanes - 1);
  const P* p = reinterpret_cast<const P*>(x + row * ld);
  auto pass = [&](auto mode, double mean) {
    constexpr int M = decltype(mode)::value;
    double a[4] = {init<M>(), init<M>(), init<M>(), init<M>()};
    int64_t c = l;
    for (; c + 3 * (int64_t)lanes < cvecs; c += 4 * (int64_t)lanes) {
      P t[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] = p[c + q * (int64_t)lanes];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < VEC; ++j) a[q] = take<M>(a[q], (double)t[q].v[j], mean);
    }
    for (; c < cvecs; c += lanes) {
      const P t = p[c];
#pragma unroll
      for (int j = 0; j < VEC; ++j) a[0] = take<M>(a[0], (double)t.v[j], mean);
    }
    double r = comb<M>(comb<M>(a[0], a[1]), comb<M>(a[2], a[3]));
    for (int off = lanes >> 1; off > 0; off >>= 1) r = comb<M>(r, __shfl_xor(r, off, kWave));
    return r;
  };
  double r = pass(std::integral_constant<int, MODE>{}, 0.0);
  if constexpr (OP == kStatVar || OP == kStatStd) {
    const double var = pass(std::integral_constant<int, kSqDev>{}, r / n) / divisor;
    r = OP == kStatStd ? sqrt(var) : var;
  }
  if (l == 0) out[row] = (T)r;
}

template <typename T, int OP>
int launch_rows(const T* x, int64_t rows, int64_t cols, int64_t ld, T* out, double divisor, hipStream_t s) {
  constexpr int N = 16 / sizeof(T);
  const bool vec = cols % N == 0 && ld % N == 0 && ((uintptr_t)x & 15) == 0;
  const int64_t cvecs = vec ? cols / N : cols;
  const int lg = log2_ceil(cvecs, 6);
  const int64_t blocks = (rows + (256 >> lg) - 1) / (256 >> lg);
  if (blocks > 0x7fffffff) return kBadArgument;
  if (vec) row_stat<T, OP, N><<<(unsigned)blocks, 256, 0, s>>>(x, rows, cvecs, ld, out, (double)cols, divisor, lg);
  else row_stat<T, OP, 1><<<(unsigned)blocks, 256, 0, s>>>(x, rows, cvecs, ld, out, (double)cols, divisor, lg);
  return launch_status();
}

struct ColPlan {
  bool vec;
  dim3 grid;
  int64_t per;
  int lgc;  // log2 of the vector kernel's column lanes per strip
};

// strips and row chunks as reduce.hip's launch_axis cuts them
template <typename T>
ColPlan plan_cols(const T* x, int64_t rows, int64_t cols, int64_t ld) {
  constexpr int V = 16 / sizeof(T);
  ColPlan p;
  p.vec = cols % V == 0 && ld % V == 0 && ((uintptr_t)x & 15) == 0 && (cols + 16 * V - 1) / (16 * V) <= kAxisTickets;
  p.lgc = log2_ceil(cols / V, 4);
  const int64_t strip = (int64_t)V << p.lgc;
  const int64_t col_blocks = p.vec ? (cols + strip - 1) / strip : (cols + 255) / 256;
  // (a table of one or two strips: 512 blocks, two per CU, where launch_axis's
  // 128 would leave half the CUs without one)
  int64_t chunks = (p.vec ? (col_blocks <= 2 ? 512 : 128) : 1024) / col_blocks;
  if (chunks * cols > kAxisWsDoubles) chunks = kAxisWsDoubles / cols;
  const int64_t min_rows = p.vec ? 1024 : 32;
  if (chunks > (rows + min_rows - 1) / min_rows) chunks = (rows + min_rows - 1) / min_rows;
  if (chunks < 1) chunks = 1;
  p.per = (rows + chunks - 1) / chunks;
  chunks = (rows + p.per - 1) / p.per;
  p.grid = dim3((unsigned)col_blocks, (unsigned)chunks);
  return p;
}

// means: the f64 column means the kSqDev pass reads (null for the others)
template <typename T, int MODE>
int launch_cols(const ColPlan& p, const T* x, int64_t rows, int64_t cols, int64_t ld, double* ws, const double* means,
                void* out, double divisor, bool root, hipStream_t s) {
  unsigned* tickets = reinterpret_cast<unsigned*>(ws + 2 * kAxisWsDoubles);
  if (p.vec)
    col_stat_v<T, MODE><<<p.grid, kColWaves * 64, 0, s>>>(x, rows, cols, ld, p.per, ws, tickets, means, out, divisor, root,
                                                          p.lgc);
  else
    col_stat<T, MODE><<<p.grid, 256, 0, s>>>(x, rows, cols, ld, p.per, ws, tickets, means, out, divisor, root);
  return launch_status();
}

template <typename T>
int launch_stat(int op, const T* x, int64_t rows, int64_t cols, int64_t ld, int axis, double divisor, T* out, double* ws,
                hipStream_t s) {
  if (axis == 1) {
    switch (op) {
      case kStatMax: return launch_rows<T, kStatMax>(x, rows, cols, ld, out, divisor, s);
      case kStatMin: return launch_rows<T, kStatMin>(x, rows, cols, ld, out, divisor, s);
      case kStatVar: return launch_rows<T, kStatVar>(x, rows, cols, ld, out, divisor, s);
      case kStatStd: return launch_rows<T, kStatStd>(x, rows, cols, ld, out, divisor, s);
    }
    return kBadArgument;
  }
  const ColPlan p = plan_cols<T>(x, rows, cols, ld);
  if (p.grid.x > kAxisTickets) return kBadArgument;
  if (op == kStatMax) return launch_cols<T, kMax>(p, x, rows, cols, ld, ws, nullptr, out, 1.0, false, s);
  if (op == kStatMin) return launch_cols<T, kMin>(p, x, rows, cols, ld, ws, nullptr, out, 1.0, false, s);
  // two launches on one stream: the f64 column means into the workspace, then
  // the squared deviations from them
  double* means = ws + kAxisWsDoubles;
  const int rc = launch_cols<T, kSum>(p, x, rows, cols, ld, ws, nullptr, means, (double)rows, false, s);
  if (rc != kOk) return rc;
  return launch_cols<T, kSqDev>(p, x, rows, cols, ld, ws, means, out, divisor, op == kStatStd, s);
}

}  // namespace axis

// partials and column means, then the tickets
WsLayout axis_stat_ws_layout() {
  const int64_t doubles = 2 * kAxisWsDoubles * (int64_t)sizeof(double);
  const int64_t tickets = kAxisTickets * (int64_t)sizeof(unsigned);
  return {doubles + tickets, doubles, tickets};
}

}  // namespace bk

using namespace bk;

// (contracts of the entry points: beekern.h)
BK_API int bk_broadcast(int op, int dtype, int kind, int swapped, const void* a, int64_t rows, int64_t cols, int64_t lda,
                        const void* v, void* y, int64_t ldy, hipStream_t stream) {
  if (!a || !v || !y || rows < 0 || cols < 0 || lda < cols || ldy < cols || op < 0 || op >= kBinCount ||
      (kind != 0 && kind != 1) || (swapped != 0 && swapped != 1) || (dtype != kF32 && dtype != kF64))
    return kBadArgument;
  if (rows == 0 || cols == 0) return kOk;
  const int64_t es = dtype_size(dtype);
  if ((((uintptr_t)a | (uintptr_t)v | (uintptr_t)y) & (uintptr_t)(es - 1)) != 0) return kBadArgument;
  uint64_t na, ny, nv;
  if (!axis::span_bytes(rows, cols, lda, es, &na) || !axis::span_bytes(rows, cols, ldy, es, &ny) ||
      __builtin_mul_overflow((uint64_t)(kind == 0 ? cols : rows), (uint64_t)es, &nv))
    return kBadArgument;
  if (axis::overlap(y, ny, v, nv)) return kBadArgument;
  if (!(y == a && ldy == lda) && axis::overlap(y, ny, a, na)) return kBadArgument;
  return dispatch_dtype<double, float>(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return dispatch_op<kBinCount>(op, [&](auto opc) {
      return dispatch_flag(kind == 0, [&](auto along_rows) {
        return dispatch_flag(swapped != 0, [&](auto swap) {
          return axis::launch_broadcast<T, decltype(opc)::value, decltype(along_rows)::value ? 0 : 1, decltype(swap)::value>(
              (const T*)a, (const T*)v, (T*)y, rows, cols, lda, ldy, stream);
        });
      });
    });
  });
}

BK_API int bk_axis_stat(int op, int dtype, const void* x, int64_t rows, int64_t cols, int64_t ld, int axis,
                        double divisor, void* out, void* ws, hipStream_t stream) {
  if (!x || !out || !ws || rows <= 0 || cols <= 0 || ld < cols || (axis != 0 && axis != 1) || op < 0 ||
      op >= axis::kStatCount || (dtype != kF32 && dtype != kF64))
    return kBadArgument;
  if ((op == axis::kStatVar || op == axis::kStatStd) && !(divisor > 0.0 && divisor <= 1.7976931348623157e308))
    return kBadArgument;
  if (axis == 0 && cols > kAxisWsDoubles) return kBadArgument;  // > 262144 columns: reduce a transposed view instead
  if (((uintptr_t)x | (uintptr_t)out) & (uintptr_t)(dtype_size(dtype) - 1)) return kBadArgument;
  if (dtype == kF64)
    return axis::launch_stat<double>(op, (const double*)x, rows, cols, ld, axis, divisor, (double*)out, (double*)ws, stream);
  return axis::launch_stat<float>(op, (const float*)x, rows, cols, ld, axis, divisor, (float*)out, (double*)ws, stream);
}
