// The sort family: bk_sort (np.sort / np.argsort(kind="stable")), bk_arg_reduce
// (np.argmax / np.argmin) and bk_take (x[int64 index]).
//
// The order is numpy's, carried by an unsigned key (bk_keys.hpp's to_key, with
// -0.0 folded onto +0.0 so the two zeros tie; int64 with its sign bit flipped):
// unsigned key order is the sorted order, every NaN has the largest key, and
// ties keep index order.
//
// bk_sort is a least-significant-digit radix sort on 8-bit digits: one counting
// launch and one scatter launch per byte of the key, buffers ping-ponging inside
// the caller's scratch.  Both launches give block b the same contiguous run of
// tiles.  The counting kernel counts the block's digits in LDS (lds_count) into a
// block-major table; the block that draws the last completion ticket
// (bk_ticket.hpp) turns the table into exclusive offsets over (digit, block).
// The scatter kernel ranks a tile stably: each wave owns a quarter of the tile
// and walks it in rows of 64 consecutive elements, a lane's rank among the
// wave's earlier equal digits comes from __ballot matching on the digit's bits
// plus the wave's running LDS count, the four waves' counts are chained in wave
// order, and the block's running offsets carry from tile to tile.
//
// No workgroup ever waits for another inside a kernel.
#include "bk_common.hpp"
#include "bk_keys.hpp"
#include "bk_ticket.hpp"

namespace bk {
namespace sort {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kDigits = 256;
constexpr int kSortRows = 16;                                   // rows of 64 elements a wave ranks per tile
constexpr int kSortTile = 4096;                                 // elements per tile: kWaves * kSortRows * 64
constexpr int kSortMaxBlocks = 512;                             // 2 per CU; the last-ticket block scans 256 x this table
constexpr int kArgMaxBlocks = 512;                              // bk_arg_reduce's grid: (key, index) partials in BK_WS_REDUCE
constexpr int kArgVecsPerLane = 4;                              // vectors a lane has before that grid grows
static_assert(kSortTile == kWaves * kSortRows * kWave, "a tile is four waves of kSortRows rows");
static_assert(kDigits == kBlock, "one thread per digit");
static_assert(2 * kArgMaxBlocks <= kRedMaxBlocks, "key and index partials share the reduction workspace's slots");

// the caller's scratch: a header (ticket, per-digit bases, the block-major table), then two key and two index buffers
constexpr int64_t kWsTicket = 0, kWsDigitBase = 256, kWsTable = kWsDigitBase + kDigits * 4;
constexpr int64_t kWsHeader = kWsTable + (int64_t)kSortMaxBlocks * kDigits * 4;
static_assert(kWsHeader % 16 == 0, "the buffers behind the header are 16-byte aligned");

inline int64_t round16(int64_t b) { return (b + 15) & ~(int64_t)15; }

// ---- keys ---------------------------------------------------------------------------
// INT: K holds an int64's bits; otherwise a float's of K's size
template <typename K, bool INT> __device__ __forceinline__ K sort_key(K u) {
  constexpr K sign = (K)((K)1 << (8 * sizeof(K) - 1));
  if constexpr (INT) return (K)(u ^ sign);
  else return to_key<K>((K)(u << 1) == 0 ? (K)0 : u);  // -0.0 ties with +0.0
}
template <typename K, bool INT> __device__ __forceinline__ K sort_value(K k) {
  constexpr K sign = (K)((K)1 << (8 * sizeof(K) - 1));
  if constexpr (INT) return (K)(k ^ sign);
  else return from_key<K>(k);
}

// the tiles of block b: [first, first + count), the same in both kernels of a pass
struct Tiles {
  int64_t first, count;
};
__device__ __forceinline__ Tiles tiles_of_block(int64_t n) {
  const int64_t ntiles = (n + kSortTile - 1) / kSortTile;
  const int64_t per = ntiles / gridDim.x, rem = ntiles % gridDim.x;
  const int64_t b = blockIdx.x;
  return Tiles{b * per + (b < rem ? b : rem), per + (b < rem ? 1 : 0)};
}

// ---- counting -------------------------------------------------------------------------
// table[b * 256 + d]: first the elements of block b with digit d, then (the
// last-ticket block) the number of elements with digit d in blocks before b;
// digit_base[d]: the number of elements with a smaller digit.
template <typename K, bool INT>
__global__ __launch_bounds__(kBlock) void sort_count(const K* __restrict__ kin, int64_t n, int shift, bool first,
                                                     unsigned* __restrict__ table, unsigned* __restrict__ digit_base,
                                                     unsigned* __restrict__ ticket) {
  __shared__ unsigned hist[kDigits];
  const int t = threadIdx.x;
  hist[t] = 0;
  __syncthreads();
  const Tiles tl = tiles_of_block(n);
  const int64_t e0 = tl.first * kSortTile;
  int64_t e1 = (tl.first + tl.count) * kSortTile;
  e1 = e1 < n ? e1 : n;
  constexpr int U = 4;
  for (int64_t i0 = e0; i0 < e1; i0 += (int64_t)U * kBlock) {  // (block-uniform trip count: lds_count ballots)
    K v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * kBlock + t;
      v[u] = i < e1 ? kin[i] : (K)0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const K key = first ? sort_key<K, INT>(v[u]) : v[u];
      lds_count(hist, (unsigned)(key >> shift) & (kDigits - 1), i0 + u * kBlock + t < e1);
    }
  }
  __syncthreads();
  publish(&table[(int64_t)blockIdx.x * kDigits + t], hist[t]);
  if (!take_last_ticket(ticket, gridDim.x)) return;

  // ---- the last block: exclusive offsets over (digit, block), thread t owning digit t ----
  const int nb = (int)gridDim.x;
  unsigned run = 0;
  constexpr int S = 8;  // table loads in flight per thread
  for (int b0 = 0; b0 < nb; b0 += S) {
    unsigned c[S];
#pragma unroll
    for (int s = 0; s < S; ++s) c[s] = b0 + s < nb ? load_agent(&table[(int64_t)(b0 + s) * kDigits + t]) : 0u;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (b0 + s < nb) publish(&table[(int64_t)(b0 + s) * kDigits + t], run);
      run += c[s];
    }
  }
  __shared__ unsigned scan[kDigits];
  scan[t] = run;
  __syncthreads();
  for (int off = 1; off < kDigits; off <<= 1) {
    const unsigned add = t >= off ? scan[t - off] : 0u;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  publish(&digit_base[t], scan[t] - run);
  if (t == 0) rearm(ticket);
}

// ---- scatter ----------------------------------------------------------------------------
// kin: this pass's keys (first: the caller's x, keyed on the fly); iin: the
// carried indices (null in the first pass: an element's index is its position,
// and null when no index is wanted).  Not last: keys to kout, indices to iout.
// Last: values to kout (the caller's sorted_out, may be null) and int64 indices
// to index_out (may be null).
template <typename K, bool INT>
__global__ __launch_bounds__(kBlock) void sort_scatter(const K* __restrict__ kin, const unsigned* __restrict__ iin,
                                                       K* __restrict__ kout, unsigned* __restrict__ iout,
                                                       long long* __restrict__ index_out, int64_t n, int shift,
                                                       bool first, bool last, bool with_index,
                                                       const unsigned* __restrict__ table,
                                                       const unsigned* __restrict__ digit_base) {
  __shared__ unsigned base[kDigits];            // where the block's next element of each digit goes
  __shared__ unsigned wcount[kWaves][kDigits];  // per wave: its count so far, then its first position, per digit
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
  volatile unsigned* mine = wcount[w];
  base[t] = digit_base[t] + table[(int64_t)blockIdx.x * kDigits + t];
  const Tiles tl = tiles_of_block(n);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t tile = tl.first; tile < tl.first + tl.count; ++tile) {
#pragma unroll
    for (int j = 0; j < kWaves; ++j) wcount[j][t] = 0;
    __syncthreads();
    const int64_t wbase = tile * kSortTile + (int64_t)w * (kSortRows * kWave) + lane;
    K key[kSortRows];
    unsigned rank[kSortRows];
#pragma unroll
    for (int r = 0; r < kSortRows; ++r) {
      const int64_t i = wbase + r * kWave;
      const K v = i < n ? kin[i] : (K)0;
      key[r] = first ? sort_key<K, INT>(v) : v;
    }
#pragma unroll
    for (int r = 0; r < kSortRows; ++r) {
      const bool valid = wbase + r * kWave < n;
      const unsigned d = (unsigned)(key[r] >> shift) & (kDigits - 1);
      // the lanes of this row with my digit
      unsigned long long peers = __ballot(valid);
#pragma unroll
      for (int bit = 0; bit < 8; ++bit) {
        const bool one = (d >> bit) & 1u;
        const unsigned long long b = __ballot(one);
        peers &= one ? b : ~b;
      }
      const unsigned before = (unsigned)__popcll(peers & below);
      // every peer reads the wave's count, then the first of them adds the row's
      unsigned prior = 0;
      if (valid) prior = mine[d];
      __builtin_amdgcn_wave_barrier();
      if (valid && before == 0) mine[d] = prior + (unsigned)__popcll(peers);
      __builtin_amdgcn_wave_barrier();
      rank[r] = prior + before;
    }
    __syncthreads();
    {  // digit t: chain the four waves, advance the block's offset
      unsigned run = base[t];
#pragma unroll
      for (int j = 0; j < kWaves; ++j) {
        const unsigned c = wcount[j][t];
        wcount[j][t] = run;
        run += c;
      }
      base[t] = run;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSortRows; ++r) {
      const int64_t i = wbase + r * kWave;
      if (i < n) {
        const unsigned d = (unsigned)(key[r] >> shift) & (kDigits - 1);
        const unsigned pos = mine[d] + rank[r];
        if (pos < (unsigned long long)n) {  // (always: the offsets partition [0, n))
          if (kout) kout[pos] = last ? sort_value<K, INT>(key[r]) : key[r];
          if (with_index) {
            const unsigned idx = first ? (unsigned)i : iin[i];
            if (last) index_out[pos] = (long long)idx;
            else iout[pos] = idx;
          }
        }
      }
    }
    __syncthreads();
  }
}

template <typename K, bool INT>
int launch_sort(const void* x, int64_t n, void* sorted_out, void* index_out, char* ws, hipStream_t q) {
  constexpr int kPasses = (int)sizeof(K);
  const bool with_index = index_out != nullptr;
  unsigned* ticket = reinterpret_cast<unsigned*>(ws + kWsTicket);
  unsigned* digit_base = reinterpret_cast<unsigned*>(ws + kWsDigitBase);
  unsigned* table = reinterpret_cast<unsigned*>(ws + kWsTable);
  const int64_t kbytes = round16(n * (int64_t)sizeof(K)), ibytes = round16(n * 4);
  K* kbuf[2] = {reinterpret_cast<K*>(ws + kWsHeader), reinterpret_cast<K*>(ws + kWsHeader + kbytes)};
  unsigned* ibuf[2] = {reinterpret_cast<unsigned*>(ws + kWsHeader + 2 * kbytes),
                       reinterpret_cast<unsigned*>(ws + kWsHeader + 2 * kbytes + ibytes)};
  // the scratch is a plain data buffer: the ticket is zeroed on the stream ahead of the first pass
  if (hipMemsetAsync(ticket, 0, 256, q) != hipSuccess) return kLaunchFailed;
  const int64_t ntiles = (n + kSortTile - 1) / kSortTile;
  const unsigned g = (unsigned)(ntiles < kSortMaxBlocks ? ntiles : kSortMaxBlocks);
  for (int p = 0; p < kPasses; ++p) {
    const bool first = p == 0, last = p == kPasses - 1;
    const K* kin = first ? (const K*)x : kbuf[(p - 1) & 1];
    const unsigned* iin = (first || !with_index) ? nullptr : ibuf[(p - 1) & 1];
    K* kout = last ? (K*)sorted_out : kbuf[p & 1];
    unsigned* iout = (last || !with_index) ? nullptr : ibuf[p & 1];
    sort_count<K, INT><<<g, kBlock, 0, q>>>(kin, n, 8 * p, first, table, digit_base, ticket);
    if (launch_status() != kOk) return kLaunchFailed;
    sort_scatter<K, INT><<<g, kBlock, 0, q>>>(kin, iin, kout, iout, last ? (long long*)index_out : nullptr, n, 8 * p,
                                               first, last, with_index, table, digit_base);
    if (launch_status() != kOk) return kLaunchFailed;
  }
  return kOk;
}

// ---- argmax / argmin -----------------------------------------------------------------------
// Both ops look for the largest 64-bit key, the smallest index among equals:
// argmax on the sort key (NaN: the largest), argmin on its complement with NaN
// still the largest (no float's key is zero, so no complement collides with it).
struct Best {
  unsigned long long key;
  long long idx;
};
__device__ __forceinline__ Best better(Best a, Best b) {
  return (b.key > a.key || (b.key == a.key && b.idx < a.idx)) ? b : a;
}
template <typename K, bool INT, bool MIN> __device__ __forceinline__ unsigned long long arg_key(K u) {
  const K k = sort_key<K, INT>(u);
  if constexpr (!MIN) return (unsigned long long)k;
  else if constexpr (INT) return (unsigned long long)(K)~k;
  else return k == (K)~(K)0 ? ~0ull : (unsigned long long)(K)~k;
}
__device__ __forceinline__ Best block_best(Best v) {
  __shared__ unsigned long long pk[kWaves];
  __shared__ long long pi[kWaves];
  auto wave = [](Best b) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      Best o;
      o.key = (unsigned long long)__shfl_xor((long long)b.key, off, kWave);
      o.idx = __shfl_xor(b.idx, off, kWave);
      b = better(b, o);
    }
    return b;
  };
  v = wave(v);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  __syncthreads();  // (called twice by the last block: the first call's reads are over)
  if (lane == 0) pk[wid] = v.key, pi[wid] = v.idx;
  __syncthreads();
  Best r{0ull, INT64_MAX};
  if (wid == 0) {
    if (lane < kWaves) r = Best{pk[lane], pi[lane]};
    r = wave(r);
  }
  return r;  // valid in thread 0
}

template <typename K, bool INT, bool MIN, bool NT>
__global__ __launch_bounds__(kBlock) void arg_reduce_kernel(const K* __restrict__ x, int64_t n, int64_t head,
                                                            unsigned long long* __restrict__ pkey,
                                                            long long* __restrict__ pidx, unsigned* __restrict__ ticket,
                                                            long long* __restrict__ out) {
  using V = V16<K>;
  constexpr int N = V::N, U = 4;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  Best best{0ull, INT64_MAX};  // (an element's index is below INT64_MAX: the first element beats it even with key 0)
  auto see = [&](int64_t i, K u) { best = better(best, Best{arg_key<K, INT, MIN>(u), (long long)i}); };
  for (int64_t k = tid; k < head; k += stride) see(k, x[k]);
  const K* xa = x + head;
  const int64_t m = n - head, nvec = m / N;
  const V* xv = reinterpret_cast<const V*>(xa);
  int64_t i = tid;
  for (; i + (U - 1) * stride < nvec; i += U * stride) {
    V v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = ld16<NT>(xv + i + u * stride);
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int j = 0; j < N; ++j) see(head + (i + u * stride) * N + j, v[u].v[j]);
    }
  }
  for (; i < nvec; i += stride) {
    const V v = xv[i];
#pragma unroll
    for (int j = 0; j < N; ++j) see(head + i * N + j, v.v[j]);
  }
  for (int64_t k = nvec * N + tid; k < m; k += stride) see(head + k, xa[k]);

  const Best mine = block_best(best);
  if (threadIdx.x == 0) {
    publish(pkey + blockIdx.x, mine.key);
    publish(pidx + blockIdx.x, mine.idx);
  }
  if (!take_last_ticket(ticket, gridDim.x)) return;
  Best r{0ull, INT64_MAX};
  for (int j = threadIdx.x; j < (int)gridDim.x; j += kBlock) r = better(r, Best{load_agent(pkey + j), load_agent(pidx + j)});
  r = block_best(r);
  if (threadIdx.x == 0) {
    *out = r.idx;
    rearm(ticket);
  }
}

template <typename K, bool INT>
int launch_arg_reduce(int op, const void* x, int64_t n, void* workspace, void* out, hipStream_t q) {
  constexpr int N = V16<K>::N;
  int64_t head = (int64_t)(((16 - ((uintptr_t)x & 15)) & 15) / sizeof(K));
  head = head < n ? head : n;
  const unsigned g = grid_blocks((n / N + kArgVecsPerLane - 1) / kArgVecsPerLane, kArgMaxBlocks);
  unsigned long long* pkey = (unsigned long long*)workspace;
  long long* pidx = (long long*)workspace + kArgMaxBlocks;
  unsigned* ticket = reinterpret_cast<unsigned*>((int64_t*)workspace + kRedMaxBlocks);
  return dispatch_flag(op == 1, [&](auto mn) {
    return dispatch_flag(stream_nt(n * (int64_t)sizeof(K)), [&](auto nt) {
      arg_reduce_kernel<K, INT, decltype(mn)::value, decltype(nt)::value>
          <<<g, kBlock, 0, q>>>((const K*)x, n, head, pkey, pidx, ticket, (long long*)out);
      return launch_status();
    });
  });
}

// ---- take -------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(kBlock) void take_kernel(const E* __restrict__ x, int64_t n, const long long* __restrict__ idx,
                                                      int64_t m, E* __restrict__ out, long long* __restrict__ partials,
                                                      unsigned* __restrict__ ticket, long long* __restrict__ bad_out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  long long bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += stride) {
    const long long j = idx[i];
    const bool ok = j >= -n && j < n;  // (n >= 0: -n does not overflow)
    E v = (E)0;
    if (ok) v = x[j < 0 ? j + n : j];
    else ++bad;
    out[i] = v;
  }
  const long long total = block_sum<long long, kBlock>(bad);
  if (threadIdx.x == 0) publish(partials + blockIdx.x, total);
  if (!take_last_ticket(ticket, gridDim.x)) return;
  long long r = 0;
  for (int j = threadIdx.x; j < (int)gridDim.x; j += kBlock) r += load_agent(partials + j);
  __syncthreads();  // (block_sum's LDS: the first call's reads are over)
  r = block_sum<long long, kBlock>(r);
  if (threadIdx.x == 0) {
    *bad_out = r;
    rearm(ticket);
  }
}

template <typename E>
int launch_take(const void* x, int64_t n, const void* idx, int64_t m, void* out, void* workspace, void* bad_out,
                hipStream_t q) {
  unsigned g = stream_grid(m, kBlock);
  g = g < (unsigned)kRedMaxBlocks ? g : (unsigned)kRedMaxBlocks;
  long long* partials = (long long*)workspace;
  unsigned* ticket = reinterpret_cast<unsigned*>((int64_t*)workspace + kRedMaxBlocks);
  take_kernel<E><<<g, kBlock, 0, q>>>((const E*)x, n, (const long long*)idx, m, (E*)out, partials, ticket,
                                      (long long*)bad_out);
  return launch_status();
}

inline bool sort_dtype(int dtype) { return dtype == kF32 || dtype == kF64 || dtype == kBF16 || dtype == kI64; }

}  // namespace sort
}  // namespace bk

using namespace bk;
using namespace bk::sort;

// (contracts of the entry points: beekern.h)
BK_API int64_t bk_sort_workspace_bytes(int dtype, int64_t n, int with_index) {
  if (!sort_dtype(dtype) || n < 0 || n > BK_MAX_SORT_N) return 0;
  return kWsHeader + 2 * round16(n * dtype_size(dtype)) + (with_index ? 2 * round16(n * 4) : 0);
}

BK_API int bk_sort(int dtype, const void* x, int64_t n, void* sorted_out, void* index_out, void* ws, int64_t ws_bytes,
                   hipStream_t stream) {
  if (!sort_dtype(dtype) || n < 0 || n > BK_MAX_SORT_N || (!sorted_out && !index_out)) return kBadArgument;
  if (n == 0) return kOk;
  if (!x || !ws || ws_bytes < bk_sort_workspace_bytes(dtype, n, index_out != nullptr)) return kBadArgument;
  const uintptr_t es = (uintptr_t)dtype_size(dtype);
  if ((uintptr_t)x % es != 0 || (uintptr_t)sorted_out % es != 0 || (uintptr_t)index_out % 8 != 0 || (uintptr_t)ws % 16 != 0)
    return kBadArgument;
  char* w = (char*)ws;
  switch (dtype) {
    case kF64: return launch_sort<uint64_t, false>(x, n, sorted_out, index_out, w, stream);
    case kI64: return launch_sort<uint64_t, true>(x, n, sorted_out, index_out, w, stream);
    case kF32: return launch_sort<uint32_t, false>(x, n, sorted_out, index_out, w, stream);
    default: return launch_sort<uint16_t, false>(x, n, sorted_out, index_out, w, stream);
  }
}

BK_API int bk_arg_reduce(int op, int dtype, const void* x, int64_t n, void* workspace, void* out, hipStream_t stream) {
  if (!x || !workspace || !out || n < 1 || op < 0 || op > 1 || !sort_dtype(dtype)) return kBadArgument;
  if ((uintptr_t)x % (uintptr_t)dtype_size(dtype) != 0 || (uintptr_t)out % 8 != 0) return kBadArgument;
  switch (dtype) {
    case kF64: return launch_arg_reduce<uint64_t, false>(op, x, n, workspace, out, stream);
    case kI64: return launch_arg_reduce<uint64_t, true>(op, x, n, workspace, out, stream);
    case kF32: return launch_arg_reduce<uint32_t, false>(op, x, n, workspace, out, stream);
    default: return launch_arg_reduce<uint16_t, false>(op, x, n, workspace, out, stream);
  }
}

BK_API int bk_take(int dtype, const void* x, int64_t n, const void* idx, int64_t m, void* out, void* workspace,
                   void* bad_out, hipStream_t stream) {
  if (!x || !idx || !out || !workspace || !bad_out || n < 0 || m < 0) return kBadArgument;
  const int es = (dtype == kF32 || dtype == kF64 || dtype == kBF16 || dtype == kBool || dtype == kI64) ? dtype_size(dtype) : 0;
  if (es == 0) return kBadArgument;
  if ((uintptr_t)x % (uintptr_t)es != 0 || (uintptr_t)out % (uintptr_t)es != 0 || (uintptr_t)idx % 8 != 0 ||
      (uintptr_t)bad_out % 8 != 0)
    return kBadArgument;
  switch (es) {
    case 8: return launch_take<uint64_t>(x, n, idx, m, out, workspace, bad_out, stream);
    case 4: return launch_take<uint32_t>(x, n, idx, m, out, workspace, bad_out, stream);
    case 2: return launch_take<uint16_t>(x, n, idx, m, out, workspace, bad_out, stream);
    default: return launch_take<uint8_t>(x, n, idx, m, out, workspace, bad_out, stream);
  }
}
