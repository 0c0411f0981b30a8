// Boolean masks: comparisons, fused compare-count, mask reductions (count /
// any / all), mask logic, where, and stable stream compaction (x[mask]).
//
// A mask is numpy's bool array: one byte per element.  Kernels WRITE exactly
// 0 or 1 and READ any non-zero byte as true (a sandbox can upload arbitrary
// bytes through the broker).  Everything here is HBM-bound: 16-byte accesses
// per lane, several in flight, non-temporal past the Infinity Cache
// (bk_common.hpp), grids from stream_grid.  Comparisons run as
// (double)a OP (double)b: the widening is exact, so this is the IEEE
// comparison of every dtype (NaN false except under !=, -0.0 == 0.0).
//
// No workgroup ever waits for another inside a kernel: the completion-ticket
// fold (bk_ticket.hpp) and kernel boundaries are the only cross-workgroup
// ordering.
#include <cstring>

#include "bk_common.hpp"
#include "bk_ticket.hpp"

namespace bk {
namespace mask {

enum CompareOp : int { kLt = 0, kLe, kGt, kGe, kEq, kNe, kCmpCount };
enum LogicalOp : int { kAnd = 0, kOr, kXor, kNot, kLogicalCount };

template <int OP> __device__ __forceinline__ bool cmp(double a, double b) {
  if constexpr (OP == kLt) return a < b;
  else if constexpr (OP == kLe) return a <= b;
  else if constexpr (OP == kGt) return a > b;
  else if constexpr (OP == kGe) return a >= b;
  else if constexpr (OP == kEq) return a == b;
  else return a != b;
}

using MaskVec = V16<uint32_t>;  // 16 mask bytes

// 0x01 in every byte of w that is non-zero (no carry crosses a byte: the low
// seven bits are summed apart from the top one)
__device__ __forceinline__ uint32_t nz_bytes(uint32_t w) {
  return ((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) >> 7) & 0x01010101u;
}
__device__ __forceinline__ unsigned count_nz(const MaskVec& m) {
  return __popc(nz_bytes(m.v[0])) + __popc(nz_bytes(m.v[1])) + __popc(nz_bytes(m.v[2])) + __popc(nz_bytes(m.v[3]));
}

// ---- compare -> mask ---------------------------------------------------------------
// A lane's 16-B vector yields only 2 / 4 / 8 mask bytes.  The block stages
// the mask bytes of one chunk (kStreamUnroll x 256 vectors) in LDS -- each lane
// writes its vector's N bytes as one 2 / 4 / 8-byte LDS store -- and writes
// them back out as coalesced 16-B global stores, so the main loop issues no
// byte-sized global store and the loads stay lane-interleaved.  Two LDS
// buffers: one barrier per chunk.
template <int N> struct MaskPiece;  // the N mask bytes of one vector
template <> struct MaskPiece<2> { using type = uint16_t; };
template <> struct MaskPiece<4> { using type = uint32_t; };
template <> struct MaskPiece<8> { using type = uint64_t; };

template <typename T, int OP, bool SCALAR, bool NT>
__global__ __launch_bounds__(256) void compare_kernel(const T* __restrict__ a, const T* __restrict__ b, double s,
                                                      uint8_t* __restrict__ y, int64_t n) {
  using V = V16<T>;
  constexpr int N = V::N, U = kStreamUnroll;
  using Piece = typename MaskPiece<N>::type;
  constexpr int kChunkBytes = U * 256 * N;       // mask bytes of one chunk
  constexpr int kChunkVecs = kChunkBytes / 16;   // 16-B mask stores of one chunk
  __shared__ __attribute__((aligned(16))) uint8_t stage[2][kChunkBytes];
  const int64_t nvec = n / N;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const V* av = reinterpret_cast<const V*>(a);
  const V* bv = reinterpret_cast<const V*>(b);
  auto piece = [&](const V& va, const V& vb) {
    Piece p = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const bool t = cmp<OP>(widen<T>(va.v[j]), SCALAR ? s : widen<T>(vb.v[j]));
      p |= (Piece)(t ? 1 : 0) << (8 * j);
    }
    return p;
  };
  const int64_t chunk = (int64_t)U * 256;
  const int64_t nfull = nvec / chunk;
  int buf = 0;
  for (int64_t cb = blockIdx.x; cb < nfull; cb += gridDim.x, buf ^= 1) {
    const int64_t base = cb * chunk + threadIdx.x;
    V va[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      va[u] = ld16<NT>(av + base + u * 256);
      if constexpr (!SCALAR) vb[u] = ld16<NT>(bv + base + u * 256);
    }
    Piece* mine = reinterpret_cast<Piece*>(stage[buf]);
#pragma unroll
    for (int u = 0; u < U; ++u) mine[u * 256 + threadIdx.x] = piece(va[u], vb[u]);
    // (the other buffer's reads, one chunk back, are behind this barrier too)
    __syncthreads();
    MaskVec* out = reinterpret_cast<MaskVec*>(y + cb * chunk * N);
    const MaskVec* src = reinterpret_cast<const MaskVec*>(stage[buf]);
#pragma unroll
    for (int q = 0; q < (kChunkVecs + 255) / 256; ++q) {
      const int i = q * 256 + threadIdx.x;
      if (kChunkVecs % 256 == 0 || i < kChunkVecs) st16<NT>(out + i, src[i]);
    }
  }
  // the vectors past the last whole chunk, then the elements past the last vector
  for (int64_t i = nfull * chunk + tid; i < nvec; i += stride) {
    V va = av[i], vb;
    if constexpr (!SCALAR) vb = bv[i];
    *reinterpret_cast<Piece*>(y + i * N) = piece(va, vb);
  }
  for (int64_t k = nvec * N + tid; k < n; k += stride)
    y[k] = cmp<OP>(widen<T>(a[k]), SCALAR ? s : widen<T>(b[k])) ? 1 : 0;
}

// ---- counts: fused compare-count, and count / any / all of a mask ------------------
// reduce.hip's stream (grid-stride, kRedBlocks blocks, 16-B loads in flight,
// f64 partials folded in index order by the last-ticket block).  Partial counts
// are integers below 2^53: the result is exact whatever the order.

enum CountKind : int { kCountCompare = 0, kCountCompareScalar, kCountMask };
enum CountFinal : int { kFinalCount = 0, kFinalAny, kFinalAll };

__device__ __forceinline__ double block_sum_f64(double v) { return block_sum<double, kRedBlock>(v); }

// fold by the last block: out = the count, or any / all of it as 0.0 / 1.0
__device__ __forceinline__ void finish_count(double v, int64_t n, int final_op, double* partials, unsigned* ticket,
                                             double* out) {
  if (threadIdx.x == 0) publish(partials + blockIdx.x, v);
  if (!take_last_ticket(ticket, gridDim.x)) return;
  const int count = (int)gridDim.x;
  double r = 0.0;
  for (int i = threadIdx.x; i < count; i += kRedBlock) r += load_agent(partials + i);
  r = block_sum_f64(r);
  if (threadIdx.x == 0) {
    if (final_op == kFinalAny) r = r > 0.0 ? 1.0 : 0.0;
    else if (final_op == kFinalAll) r = r == (double)n ? 1.0 : 0.0;
    *out = r;
    rearm(ticket);
  }
}

// T: the element type (uint32_t words of a mask for kCountMask, 16 bytes a vector)
template <typename T, int OP, int KIND, bool NT, int U>
__global__ __launch_bounds__(kRedBlock) void count_kernel(const T* __restrict__ a, const T* __restrict__ b, double s,
                                                          int64_t n, int final_op, double* __restrict__ partials,
                                                          unsigned* __restrict__ ticket, double* __restrict__ out) {
  using V = V16<T>;
  constexpr bool kMask = KIND == kCountMask, kScalar = KIND == kCountCompareScalar;
  constexpr int N = kMask ? 16 : V::N;  // elements per vector
  const int64_t nvec = n / N;
  const int64_t stride = (int64_t)gridDim.x * kRedBlock;
  const int64_t tid = (int64_t)blockIdx.x * kRedBlock + threadIdx.x;
  const V* av = reinterpret_cast<const V*>(a);
  const V* bv = reinterpret_cast<const V*>(b);
  auto count = [&](const V& va, const V& vb) -> unsigned {
    if constexpr (kMask) {
      return count_nz(reinterpret_cast<const MaskVec&>(va));
    } else {
      unsigned c = 0;
#pragma unroll
      for (int j = 0; j < V::N; ++j) c += cmp<OP>(widen<T>(va.v[j]), kScalar ? s : widen<T>(vb.v[j])) ? 1u : 0u;
      return c;
    }
  };
  // per-lane counts: at most n / (lanes of the grid) + a tail, far below 2^32
  unsigned acc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) acc[u] = 0;
  int64_t i = tid;
  for (; i + (U - 1) * stride < nvec; i += U * stride) {
    V va[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      va[u] = ld16<NT>(av + i + u * stride);
      if constexpr (KIND == kCountCompare) vb[u] = ld16<NT>(bv + i + u * stride);
    }
    // every load is issued before the first count: the comparisons land in
    // scalar registers, and the scheduler otherwise sinks each load to its
    // use to save them (one or two loads in flight instead of U)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] += count(va[u], vb[u]);
  }
  constexpr int U2 = 4;
  for (; i + (U2 - 1) * stride < nvec; i += U2 * stride) {
    V va[U2], vb[U2];
#pragma unroll
    for (int u = 0; u < U2; ++u) {
      va[u] = ld16<NT>(av + i + u * stride);
      if constexpr (KIND == kCountCompare) vb[u] = ld16<NT>(bv + i + u * stride);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U2; ++u) acc[u] += count(va[u], vb[u]);
  }
  for (; i < nvec; i += stride) {
    V va = av[i], vb;
    if constexpr (KIND == kCountCompare) vb = bv[i];
    acc[0] += count(va, vb);
  }
  for (int64_t k = nvec * N + tid; k < n; k += stride) {
    if constexpr (kMask) acc[0] += reinterpret_cast<const uint8_t*>(a)[k] != 0 ? 1u : 0u;
    else acc[0] += cmp<OP>(widen<T>(a[k]), kScalar ? s : widen<T>(b[k])) ? 1u : 0u;
  }
  uint64_t c = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) c += acc[u];
  finish_count(block_sum_f64((double)c), n, final_op, partials, ticket, out);
}

template <typename T, int OP, int KIND>
int launch_count(const void* a, const void* b, double s, int64_t n, int final_op, double* ws, double* out,
                 hipStream_t q) {
  constexpr int N = KIND == kCountMask ? 16 : 16 / (int)sizeof(T);
  constexpr int64_t esize = KIND == kCountMask ? 1 : (int64_t)sizeof(T);
  // two-operand streams keep 8 vectors of each operand in flight (the register budget of 16 of one)
  constexpr int U = KIND == kCountCompare ? 8 : 16;
  // 4 vectors per lane before adding blocks, as launch_reduce; the default grid whatever BK_REDUCE_BLOCKS says
  const unsigned g = grid_blocks((n / N + 3) / 4, kRedBlocks);
  unsigned* ticket = reinterpret_cast<unsigned*>(ws + kRedMaxBlocks);
  return dispatch_flag(stream_nt(n * esize * (KIND == kCountCompare ? 2 : 1)), [&](auto nt) {
    count_kernel<T, OP, KIND, decltype(nt)::value, U>
        <<<g, kRedBlock, 0, q>>>((const T*)a, (const T*)b, s, n, final_op, ws, ticket, out);
    return launch_status();
  });
}

template <typename T, int OP>
int launch_compare(int mode, const void* a, const void* b, double s, void* y, int64_t n, hipStream_t q) {
  constexpr int N = 16 / (int)sizeof(T);
  // whole chunks per block: the grid never exceeds the chunk count by much
  const int64_t chunks = (n / N) / (kStreamUnroll * 256);
  const unsigned g = stream_grid((chunks > 0 ? chunks : 1) * 256, 256);
  return dispatch_flag(mode == 0, [&](auto arrays) {
    return dispatch_flag(stream_nt(n * (int64_t)sizeof(T) * (mode == 0 ? 2 : 1)), [&](auto nt) {
      compare_kernel<T, OP, !decltype(arrays)::value, decltype(nt)::value>
          <<<g, 256, 0, q>>>((const T*)a, (const T*)b, s, (uint8_t*)y, n);
      return launch_status();
    });
  });
}

// ---- mask logic --------------------------------------------------------------------
constexpr int kLogicUnroll = 4;

template <int OP> __device__ __forceinline__ uint32_t logic_word(uint32_t a, uint32_t b) {
  if constexpr (OP == kAnd) return nz_bytes(a) & nz_bytes(b);
  else if constexpr (OP == kOr) return nz_bytes(a | b);
  else if constexpr (OP == kXor) return nz_bytes(a) ^ nz_bytes(b);
  else return nz_bytes(a) ^ 0x01010101u;
}

template <int OP, bool NT>
__global__ __launch_bounds__(256) void logical_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                      uint8_t* __restrict__ y, int64_t n) {
  constexpr int U = kLogicUnroll;
  constexpr bool kTwo = OP != kNot;
  const int64_t nvec = n / 16;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const MaskVec* av = reinterpret_cast<const MaskVec*>(a);
  const MaskVec* bv = reinterpret_cast<const MaskVec*>(b);
  MaskVec* yv = reinterpret_cast<MaskVec*>(y);
  auto apply = [&](MaskVec& va, const MaskVec& vb) {
#pragma unroll
    for (int j = 0; j < 4; ++j) va.v[j] = logic_word<OP>(va.v[j], kTwo ? vb.v[j] : 0u);
  };
  const int64_t chunk = (int64_t)U * 256;
  const int64_t nfull = nvec / chunk;
  for (int64_t cb = blockIdx.x; cb < nfull; cb += gridDim.x) {
    const int64_t base = cb * chunk + threadIdx.x;
    MaskVec va[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      va[u] = ld16<NT>(av + base + u * 256);
      if constexpr (kTwo) vb[u] = ld16<NT>(bv + base + u * 256);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) apply(va[u], vb[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) st16<NT>(yv + base + u * 256, va[u]);
  }
  for (int64_t i = nfull * chunk + tid; i < nvec; i += stride) {
    MaskVec va = av[i], vb;
    if constexpr (kTwo) vb = bv[i];
    apply(va, vb);
    yv[i] = va;
  }
  for (int64_t k = nvec * 16 + tid; k < n; k += stride)
    y[k] = (uint8_t)logic_word<OP>(a[k], kTwo ? b[k] : 0u);
}

template <int OP>
int launch_logical(const void* a, const void* b, void* y, int64_t n, hipStream_t q) {
  const unsigned g = stream_grid((n + 15) / 16, 256);
  return dispatch_flag(stream_nt(n), [&](auto nt) {
    logical_kernel<OP, decltype(nt)::value><<<g, 256, 0, q>>>((const uint8_t*)a, (const uint8_t*)b, (uint8_t*)y, n);
    return launch_status();
  });
}

// ---- where -------------------------------------------------------------------------
// out[i] = mask[i] ? A : B, values moved as bits (T: the 2 / 4 / 8-byte
// unsigned integer of the dtype's size).  A lane owns one 16-B vector of the
// output and the N mask bytes that go with it (one 2 / 4 / 8-byte load).
template <typename T, bool A_SCALAR, bool B_SCALAR, bool NT>
__global__ __launch_bounds__(256) void where_kernel(const uint8_t* __restrict__ m, const T* __restrict__ a,
                                                    const T* __restrict__ b, T sa, T sb, T* __restrict__ y,
                                                    int64_t n) {
  using V = V16<T>;
  constexpr int N = V::N, U = kStreamUnroll;
  using Piece = typename MaskPiece<N>::type;
  const int64_t nvec = n / N;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const V* av = reinterpret_cast<const V*>(a);
  const V* bv = reinterpret_cast<const V*>(b);
  const Piece* mv = reinterpret_cast<const Piece*>(m);
  V* yv = reinterpret_cast<V*>(y);
  auto select = [&](Piece p, const V& va, const V& vb) {
    V r;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const bool t = ((p >> (8 * j)) & 0xff) != 0;
      r.v[j] = t ? (A_SCALAR ? sa : va.v[j]) : (B_SCALAR ? sb : vb.v[j]);
    }
    return r;
  };
  const int64_t chunk = (int64_t)U * 256;
  const int64_t nfull = nvec / chunk;
  for (int64_t cb = blockIdx.x; cb < nfull; cb += gridDim.x) {
    const int64_t base = cb * chunk + threadIdx.x;
    V va[U], vb[U];
    Piece p[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      p[u] = mv[base + u * 256];
      if constexpr (!A_SCALAR) va[u] = ld16<NT>(av + base + u * 256);
      if constexpr (!B_SCALAR) vb[u] = ld16<NT>(bv + base + u * 256);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) st16<NT>(yv + base + u * 256, select(p[u], va[u], vb[u]));
  }
  for (int64_t i = nfull * chunk + tid; i < nvec; i += stride) {
    V va, vb;
    if constexpr (!A_SCALAR) va = av[i];
    if constexpr (!B_SCALAR) vb = bv[i];
    yv[i] = select(mv[i], va, vb);
  }
  for (int64_t k = nvec * N + tid; k < n; k += stride)
    y[k] = m[k] != 0 ? (A_SCALAR ? sa : a[k]) : (B_SCALAR ? sb : b[k]);
}

template <typename T>
int launch_where(const void* m, int flags, const void* a, const void* b, T sa, T sb, void* y, int64_t n,
                 hipStream_t q) {
  const unsigned g = stream_grid((n + V16<T>::N - 1) / V16<T>::N, 256);
  // flags bit 0: A is the scalar sa, bit 1: B is the scalar sb
  return dispatch_flag(!(flags & 2), [&](auto b_array) {
    return dispatch_flag(!(flags & 1), [&](auto a_array) {
      return dispatch_flag(stream_nt(n * (int64_t)sizeof(T)), [&](auto nt) {
        where_kernel<T, !decltype(a_array)::value, !decltype(b_array)::value, decltype(nt)::value>
            <<<g, 256, 0, q>>>((const uint8_t*)m, (const T*)a, (const T*)b, sa, sb, (T*)y, n);
        return launch_status();
      });
    });
  });
}

// host-side RNE f32 -> bf16 bits (NaN -> quiet NaN), as float_to_bf16_bits
inline uint16_t host_bf16_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x007fffffu)) return 0x7fc0;
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// ---- stable compaction: out = x[mask] in index order ------------------------------
// The array is cut into tiles of kTile elements; a capped grid of blocks each
// owns a contiguous run of whole tiles (the workspace is sized by the cap).
//   launch 1: every block counts the true bytes of its run (16-B mask loads)
//             and publishes the count; the block that draws the last ticket
//             turns the counts into exclusive offsets.
//   launch 2: every block walks its run tile by tile.  A wave owns 64 * kCzU
//             consecutive elements of the tile: per step each lane takes one
//             element, __ballot (64-bit) + popcount of the lanes below rank
//             it, the waves' tile counts go through LDS for the per-wave
//             offsets, and the selected elements are scattered.  An index at
//             or past `cap` is dropped.
constexpr int kCzBlock = 256;
constexpr int kCzWaves = kCzBlock / kWave;
constexpr int kCzU = 16;                        // steps of one wave per tile, loads in flight per lane
constexpr int kTile = kCzBlock * kCzU;          // 4096 elements
constexpr int kCzMaxBlocks = 2048;              // 8 per CU
// workspace: counts[kCzMaxBlocks], offsets[kCzMaxBlocks] (u64), then the ticket's 256 B
constexpr int64_t kCzWsBytes = 2ll * kCzMaxBlocks * 8 + 256;

struct CzPlan {
  unsigned grid;
  int64_t per;  // elements of a block's run (whole tiles)
};
inline CzPlan cz_plan(int64_t n) {
  const int64_t tiles = (n + kTile - 1) / kTile;
  const int64_t tiles_per = (tiles + kCzMaxBlocks - 1) / kCzMaxBlocks;
  return CzPlan{(unsigned)((tiles + tiles_per - 1) / tiles_per), tiles_per * kTile};
}

template <bool NT>
__global__ __launch_bounds__(kCzBlock) void compress_count(const uint8_t* __restrict__ m, int64_t n, int64_t per,
                                                           unsigned long long* __restrict__ counts,
                                                           unsigned long long* __restrict__ offsets,
                                                           unsigned* __restrict__ ticket) {
  const int64_t s0 = (int64_t)blockIdx.x * per;
  const int64_t s1 = s0 + per < n ? s0 + per : n;
  // (s0 is a multiple of kTile: 16-B aligned whenever the mask is)
  const MaskVec* mv = reinterpret_cast<const MaskVec*>(m + s0);
  const int64_t nvec = (s1 - s0) / 16;
  unsigned c = 0;
  int64_t i = threadIdx.x;
  for (; i + 3 * kCzBlock < nvec; i += 4 * kCzBlock) {
    MaskVec v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = ld16<NT>(mv + i + u * kCzBlock);
#pragma unroll
    for (int u = 0; u < 4; ++u) c += count_nz(v[u]);
  }
  for (; i < nvec; i += kCzBlock) c += count_nz(mv[i]);
  for (int64_t k = s0 + nvec * 16 + threadIdx.x; k < s1; k += kCzBlock) c += m[k] != 0 ? 1u : 0u;
  const unsigned total = block_sum<unsigned, kCzBlock>(c);
  if (threadIdx.x == 0) publish(counts + blockIdx.x, (unsigned long long)total);
  if (!take_last_ticket(ticket, gridDim.x)) return;
  // exclusive scan of <= kCzMaxBlocks counts: 8 consecutive counts per thread,
  // then a Hillis-Steele scan of the 256 thread sums in LDS
  constexpr int kPer = kCzMaxBlocks / kCzBlock;
  __shared__ unsigned long long scan[kCzBlock];
  const int blocks = (int)gridDim.x;
  unsigned long long mine[kPer], sum = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int idx = threadIdx.x * kPer + j;
    mine[j] = idx < blocks ? load_agent(counts + idx) : 0ull;
    sum += mine[j];
  }
  scan[threadIdx.x] = sum;
  __syncthreads();
  for (int off = 1; off < kCzBlock; off <<= 1) {
    const unsigned long long t = (int)threadIdx.x >= off ? scan[threadIdx.x - off] : 0ull;
    __syncthreads();
    scan[threadIdx.x] += t;
    __syncthreads();
  }
  unsigned long long run = scan[threadIdx.x] - sum;  // exclusive
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int idx = threadIdx.x * kPer + j;
    if (idx < blocks) offsets[idx] = run;  // (read by the next launch: a kernel boundary orders it)
    run += mine[j];
  }
  if (threadIdx.x == 0) rearm(ticket);
}

template <typename T>
__global__ __launch_bounds__(kCzBlock) void compress_scatter(const T* __restrict__ x, const uint8_t* __restrict__ m,
                                                             int64_t n, int64_t per,
                                                             const unsigned long long* __restrict__ offsets,
                                                             T* __restrict__ out, int64_t cap) {
  __shared__ unsigned wave_count[kCzWaves];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int64_t s0 = (int64_t)blockIdx.x * per;
  const int64_t s1 = s0 + per < n ? s0 + per : n;
  int64_t pos = (int64_t)offsets[blockIdx.x];  // output index of this block's next true element
  for (int64_t t0 = s0; t0 < s1; t0 += kTile) {  // (block-uniform trip count: the barriers below are safe)
    const int64_t w0 = t0 + (int64_t)wid * kWave * kCzU + lane;
    bool sel[kCzU];
    T val[kCzU];
    if (t0 + kTile <= s1) {
      // a whole tile: every mask byte and every element loaded unguarded,
      // all in flight (a load under its own branch waits for the one before)
      uint8_t mb[kCzU];
#pragma unroll
      for (int u = 0; u < kCzU; ++u) mb[u] = m[w0 + u * kWave];
#pragma unroll
      for (int u = 0; u < kCzU; ++u) val[u] = x[w0 + u * kWave];
#pragma unroll
      for (int u = 0; u < kCzU; ++u) sel[u] = mb[u] != 0;
    } else {
      // the ragged last tile of the array: nothing past s1 (<= n) is read
#pragma unroll
      for (int u = 0; u < kCzU; ++u) {
        const int64_t i = w0 + u * kWave;
        sel[u] = false;
        if (i < s1) {
          sel[u] = m[i] != 0;
          val[u] = x[i];
        }
      }
    }
    unsigned long long bal[kCzU];
    unsigned mine = 0;
#pragma unroll
    for (int u = 0; u < kCzU; ++u) {
      bal[u] = __ballot(sel[u]);
      mine += (unsigned)__popcll(bal[u]);
    }
    if (lane == 0) wave_count[wid] = mine;
    __syncthreads();
    int64_t at = pos;
    unsigned tile_total = 0;
#pragma unroll
    for (int w = 0; w < kCzWaves; ++w) {
      const unsigned cw = wave_count[w];
      if (w < wid) at += cw;
      tile_total += cw;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int u = 0; u < kCzU; ++u) {
      const int64_t o = at + __popcll(bal[u] & below);
      if (sel[u] && o < cap) out[o] = val[u];
      at += __popcll(bal[u]);
    }
    pos += tile_total;
    __syncthreads();  // wave_count is rewritten by the next tile
  }
}

template <typename T>
int launch_compress(const void* x, const void* m, int64_t n, void* out, int64_t cap, void* ws, hipStream_t q) {
  const CzPlan plan = cz_plan(n);
  unsigned long long* counts = (unsigned long long*)ws;
  unsigned long long* offsets = counts + kCzMaxBlocks;
  unsigned* ticket = reinterpret_cast<unsigned*>(offsets + kCzMaxBlocks);
  const int rc = dispatch_flag(stream_nt(n), [&](auto nt) {
    compress_count<decltype(nt)::value>
        <<<plan.grid, kCzBlock, 0, q>>>((const uint8_t*)m, n, plan.per, counts, offsets, ticket);
    return launch_status();
  });
  if (rc != kOk) return rc;
  compress_scatter<T><<<plan.grid, kCzBlock, 0, q>>>((const T*)x, (const uint8_t*)m, n, plan.per, offsets, (T*)out, cap);
  return launch_status();
}

}  // namespace mask

// bk_reduce on kBool (reduce.hip forwards it): op 0 count, 3 any, 4 all
int reduce_bool(int op, const void* a, int64_t n, void* workspace, void* out, hipStream_t stream) {
  using namespace mask;
  const int final_op = op == 0 ? kFinalCount : op == 3 ? kFinalAny : op == 4 ? kFinalAll : -1;
  if (final_op < 0) return kBadArgument;
  return launch_count<uint32_t, 0, kCountMask>(a, nullptr, 0.0, n, final_op, (double*)workspace, (double*)out, stream);
}

// counts and offsets, then the ticket's 256 B
WsLayout compress_ws_layout() { return {mask::kCzWsBytes, 2ll * mask::kCzMaxBlocks * 8, 256}; }

}  // namespace bk

using namespace bk;
using namespace bk::mask;

// (contracts of the entry points: beekern.h)
BK_API int bk_compare(int op, int dtype, int mode, const void* a, const void* b, double scalar, void* mask_out,
                      int64_t n, hipStream_t stream) {
  if (!a || !mask_out || n < 0 || op < 0 || op >= kCmpCount || mode < 0 || mode > 1 || (mode == 0 && !b))
    return kBadArgument;
  if (dtype != kF32 && dtype != kF64 && dtype != kBF16) return kBadArgument;
  if (n == 0) return kOk;
  return dispatch_dtype<float, double, uint16_t>(dtype, [&](auto t) {
    return dispatch_op<kCmpCount>(op, [&](auto opc) {
      return launch_compare<typename decltype(t)::type, decltype(opc)::value>(mode, a, b, scalar, mask_out, n, stream);
    });
  });
}

BK_API int bk_compare_count(int op, int dtype, int mode, const void* a, const void* b, double scalar, int64_t n,
                            void* workspace, void* out, hipStream_t stream) {
  if (!a || !workspace || !out || n < 0 || op < 0 || op >= kCmpCount || mode < 0 || mode > 1 || (mode == 0 && !b))
    return kBadArgument;
  return dispatch_dtype<float, double, uint16_t>(dtype, [&](auto t) {
    return dispatch_op<kCmpCount>(op, [&](auto opc) {
      return dispatch_flag(mode == 0, [&](auto arrays) {
        constexpr int KIND = decltype(arrays)::value ? kCountCompare : kCountCompareScalar;
        return launch_count<typename decltype(t)::type, decltype(opc)::value, KIND>(
            a, b, scalar, n, kFinalCount, (double*)workspace, (double*)out, stream);
      });
    });
  });
}

BK_API int bk_mask_logical(int op, const void* a, const void* b, void* out, int64_t n, hipStream_t stream) {
  if (!a || !out || n < 0 || op < 0 || op >= kLogicalCount || (op != kNot && !b)) return kBadArgument;
  if (n == 0) return kOk;
  switch (op) {
    case kAnd: return launch_logical<kAnd>(a, b, out, n, stream);
    case kOr: return launch_logical<kOr>(a, b, out, n, stream);
    case kXor: return launch_logical<kXor>(a, b, out, n, stream);
    default: return launch_logical<kNot>(a, nullptr, out, n, stream);
  }
}

BK_API int bk_where(int dtype, const void* mask, int flags, const void* a, const void* b, double sa, double sb,
                    void* out, int64_t n, hipStream_t stream) {
  if (!mask || !out || n < 0 || (flags & ~3) != 0 || (!(flags & 1) && !a) || (!(flags & 2) && !b)) return kBadArgument;
  if (dtype != kF32 && dtype != kF64 && dtype != kBF16) return kBadArgument;
  if (n == 0) return kOk;
  if (dtype == kF64) {
    uint64_t ua, ub;
    memcpy(&ua, &sa, 8);
    memcpy(&ub, &sb, 8);
    return launch_where<uint64_t>(mask, flags, a, b, ua, ub, out, n, stream);
  }
  const float fa = (float)sa, fb = (float)sb;
  if (dtype == kF32) {
    uint32_t ua, ub;
    memcpy(&ua, &fa, 4);
    memcpy(&ub, &fb, 4);
    return launch_where<uint32_t>(mask, flags, a, b, ua, ub, out, n, stream);
  }
  return launch_where<uint16_t>(mask, flags, a, b, host_bf16_bits(fa), host_bf16_bits(fb), out, n, stream);
}

BK_API int bk_compress(int dtype, const void* x, const void* mask, int64_t n, void* out, int64_t cap, void* workspace,
                       hipStream_t stream) {
  if (!x || !mask || !out || !workspace || n < 0 || cap < 0) return kBadArgument;
  if (dtype != kF32 && dtype != kF64 && dtype != kBF16 && dtype != kBool) return kBadArgument;
  if (n == 0) return kOk;
  switch (dtype) {
    case kF64: return launch_compress<uint64_t>(x, mask, n, out, cap, workspace, stream);
    case kF32: return launch_compress<uint32_t>(x, mask, n, out, cap, workspace, stream);
    case kBF16: return launch_compress<uint16_t>(x, mask, n, out, cap, workspace, stream);
    default: return launch_compress<uint8_t>(x, mask, n, out, cap, workspace, stream);
  }
}
