// Order statistics and histograms: bk_select (the k-th smallest elements, by
// radix select) and bk_histogram (numpy's np.histogram counts).
//
// Both are one primitive: every workgroup counts its share of the array into
// a histogram in LDS, adds the non-zero counts to a table in global memory,
// and the workgroup that draws the last completion ticket (bk_ticket.hpp)
// reads the merged table.  The array is only ever read: 16-byte loads, several
// in flight, non-temporal past the Infinity Cache (bk_common.hpp).
//
// The LDS counts are u32 atomics.  A wave whose lanes all hit one counter
// (all-equal data; the top byte of uniform [0, 1) doubles) would serialise on
// that address, so lds_count (bk_keys.hpp) first peels the wave's most common indices:
// the lanes that share the first active lane's index add their number once
// (__ballot + popcount), twice over, and only what is left adds lane by lane.
//
// No workgroup ever waits for another inside a kernel.
#include <cstring>

#include "bk_common.hpp"
#include "bk_keys.hpp"
#include "bk_ticket.hpp"

namespace bk {
namespace stats {

constexpr int kBlock = 256;
constexpr int kUnroll = 4;          // 16-B loads in flight per lane
constexpr int kMaxBlocks = 1024;    // 4 per CU; every block merges its counts into the table once

constexpr int kMaxRanks = BK_MAX_RANKS;
constexpr int kDigitBits = 8;
constexpr int kDigits = 1 << kDigitBits;

constexpr int kMaxBins = BK_MAX_BINS;

// Calls f(element bits) for every element of x[0:n), all lanes of a block
// walking the same whole chunks (kUnroll x kBlock vectors: the block's tile).
// `head`: the elements before the first 16-byte boundary.
template <typename K, bool NT, typename F>
__device__ __forceinline__ void for_each_element(const K* __restrict__ x, int64_t n, int64_t head, F&& f) {
  using V = V16<K>;
  constexpr int N = V::N;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  for (int64_t k = tid; k < head; k += stride) f(x[k]);
  const K* xa = x + head;
  const int64_t m = n - head;
  const int64_t nvec = m / N;
  const V* xv = reinterpret_cast<const V*>(xa);
  const int64_t chunk = (int64_t)kUnroll * kBlock;
  const int64_t nfull = nvec / chunk;
  for (int64_t cb = blockIdx.x; cb < nfull; cb += gridDim.x) {
    const int64_t base = cb * chunk + threadIdx.x;
    V v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) v[u] = ld16<NT>(xv + base + u * kBlock);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
      for (int j = 0; j < N; ++j) f(v[u].v[j]);
    }
  }
  for (int64_t i = nfull * chunk + tid; i < nvec; i += stride) {
    const V v = xv[i];
#pragma unroll
    for (int j = 0; j < N; ++j) f(v.v[j]);
  }
  for (int64_t k = nvec * N + tid; k < m; k += stride) f(xa[k]);
}

// elements of one block's tile, per dtype size (tests/test_stats_gpu.py sizes around it)
template <typename K> constexpr int64_t tile_elements() { return (int64_t)kUnroll * kBlock * V16<K>::N; }

template <typename K>
inline unsigned grid_for(int64_t n) {
  const int64_t tiles = (n + tile_elements<K>() - 1) / tile_elements<K>();
  return (unsigned)(tiles < 1 ? 1 : tiles < kMaxBlocks ? tiles : kMaxBlocks);
}

template <typename K>
inline int64_t head_elements(const void* x, int64_t n) {
  const int64_t h = (int64_t)(((16 - ((uintptr_t)x & 15)) & 15) / sizeof(K));
  return h < n ? h : n;
}

// ---- keys ---------------------------------------------------------------------------
// (to_key / from_key: bk_keys.hpp)
__device__ __forceinline__ double bits_to_double(uint64_t b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ double bits_to_double(uint32_t b) { return (double)__uint_as_float(b); }
__device__ __forceinline__ double bits_to_double(uint16_t b) { return (double)bf16_bits_to_float(b); }

// ---- radix select -------------------------------------------------------------------
// One launch per 8-bit digit of the key, most significant first.  The state
// between launches lives in the workspace: the ranks are kept in groups that
// share the key prefix found so far (one histogram per group: adjacent ranks
// -- the two neighbours an interpolated quantile needs -- stay one group until
// their keys part), each rank with its remaining rank inside its group's
// prefix.  The last-ticket block scans each group's merged counts, gives
// every rank its next digit, regroups, clears the table and re-arms the
// ticket; after the last digit it writes the values.
struct SelectWs {
  unsigned long long table[kMaxRanks * kDigits];  // merged counts, group-major; zero between launches
  unsigned long long prefix[kMaxRanks];           // per group: the key bits fixed so far (the rest zero)
  unsigned long long rem[kMaxRanks];              // per rank: its rank among the elements with its group's prefix
  unsigned group[kMaxRanks];                      // per rank
  unsigned ngroups;
  unsigned pad;
  unsigned long long nan;                         // NaNs seen by the first pass; zero between calls
  alignas(256) unsigned ticket[64];
};

struct Ranks {
  long long k[kMaxRanks];
};

// a block-uniform value into scalar registers
__device__ __forceinline__ uint64_t uniform(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint16_t uniform(uint16_t v) { return (uint16_t)__builtin_amdgcn_readfirstlane((int)v); }

// One pass's counting: every element whose bits above the digit equal a
// group's prefix counts its digit into that group's histogram (groups have
// distinct prefixes: at most one matches).  MAXG > 0: ng <= MAXG, prefixes in
// registers; MAXG == 0: any ng, prefixes read from LDS.  Returns this lane's
// NaN count (first pass only).
template <typename K, bool NT, int MAXG>
__device__ __forceinline__ unsigned count_digits(const K* __restrict__ x, int64_t n, int64_t head, int pass, int shift,
                                                 K himask, int ng, const K* s_prefix, unsigned* hist) {
  unsigned nans = 0;
  // (a prefix has the digit's bits and those below it zero, as key & himask
  // has: all-ones, for the slots past ng, equals none)
  K pre[MAXG > 0 ? MAXG : 1];
#pragma unroll
  for (int j = 0; j < (MAXG > 0 ? MAXG : 1); ++j) pre[j] = j < ng ? uniform(s_prefix[j]) : (K)~(K)0;
  for_each_element<K, NT>(x, n, head, [&](K u) {
    const K key = to_key<K>(u);
    if (pass == 0) nans += key == (K)~(K)0 ? 1u : 0u;
    const K above = (K)(key & himask);  // one compare per group: the loop is VALU-bound, not HBM-bound, otherwise
    int g = -1;
    if constexpr (MAXG > 0) {
#pragma unroll
      for (int j = 0; j < MAXG; ++j) g = above == pre[j] ? j : g;
    } else {
      for (int j = 0; j < ng; ++j) g = above == s_prefix[j] ? j : g;
    }
    const unsigned digit = (unsigned)(key >> shift) & (kDigits - 1);
    lds_count(hist, (unsigned)(g < 0 ? 0 : g) * kDigits + digit, g >= 0);
  });
  return nans;
}

template <typename K, bool NT>
__global__ __launch_bounds__(kBlock) void select_pass(const K* __restrict__ x, int64_t n, int64_t head, int pass,
                                                      int nranks, Ranks ranks, SelectWs* __restrict__ ws,
                                                      double* __restrict__ out) {
  constexpr int kPasses = (int)sizeof(K);
  __shared__ unsigned hist[kMaxRanks * kDigits];
  __shared__ K s_prefix[kMaxRanks];
  const int shift = kDigitBits * (kPasses - 1 - pass);
  // the bits above this pass's digit (none in the first pass: every element is in group 0)
  const K himask = pass == 0 ? (K)0 : (K)((K)~(K)0 << (shift + kDigitBits));
  int ng = pass == 0 ? 1 : (int)ws->ngroups;
  ng = ng < 1 ? 1 : ng > kMaxRanks ? kMaxRanks : ng;
  if ((int)threadIdx.x < ng) s_prefix[threadIdx.x] = pass == 0 ? (K)0 : (K)ws->prefix[threadIdx.x];
  for (int i = threadIdx.x; i < ng * kDigits; i += kBlock) hist[i] = 0;
  __syncthreads();

  // up to 2 groups (a median, one interpolated quantile), up to 8 and up to
  // 16 keep the prefixes in scalar registers; more are matched against LDS
  unsigned nans;
  if (ng <= 2) nans = count_digits<K, NT, 2>(x, n, head, pass, shift, himask, ng, s_prefix, hist);
  else if (ng <= 8) nans = count_digits<K, NT, 8>(x, n, head, pass, shift, himask, ng, s_prefix, hist);
  else if (ng <= 16) nans = count_digits<K, NT, 16>(x, n, head, pass, shift, himask, ng, s_prefix, hist);
  else nans = count_digits<K, NT, 0>(x, n, head, pass, shift, himask, ng, s_prefix, hist);
  __syncthreads();
  for (int i = threadIdx.x; i < ng * kDigits; i += kBlock) {
    const unsigned c = hist[i];
    if (c) __hip_atomic_fetch_add(&ws->table[i], (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (pass == 0) {
    const unsigned total = block_sum<unsigned, kBlock>(nans);
    if (threadIdx.x == 0 && total)
      __hip_atomic_fetch_add(&ws->nan, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!take_last_ticket(ws->ticket, gridDim.x)) return;

  // ---- the last block: every rank's next digit ----
  __shared__ unsigned long long scan[kBlock];
  __shared__ unsigned long long s_rem[kMaxRanks], s_newrem[kMaxRanks];
  __shared__ K s_np[kMaxRanks];
  __shared__ int s_group[kMaxRanks], s_digit[kMaxRanks], s_leader[kMaxRanks];
  static_assert(kDigits == kBlock, "one thread per digit");
  const int t = threadIdx.x;
  if (t < nranks) {
    s_rem[t] = pass == 0 ? (unsigned long long)ranks.k[t] : ws->rem[t];
    const int g = pass == 0 ? 0 : (int)ws->group[t];
    s_group[t] = g < 0 ? 0 : g >= ng ? ng - 1 : g;
    s_digit[t] = 0;
    s_newrem[t] = 0;
  }
  __syncthreads();
  for (int g = 0; g < ng; ++g) {
    const unsigned long long c = load_agent(&ws->table[g * kDigits + t]);
    publish(&ws->table[g * kDigits + t], 0ull);
    scan[t] = c;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
      const unsigned long long add = t >= off ? scan[t - off] : 0ull;
      __syncthreads();
      scan[t] += add;
      __syncthreads();
    }
    const unsigned long long incl = scan[t], excl = incl - c;
    for (int r = 0; r < nranks; ++r) {
      if (s_group[r] != g) continue;
      const unsigned long long k = s_rem[r];
      if (excl <= k && k < incl) {  // exactly one digit holds the rank (k < the group's total)
        s_digit[r] = t;
        s_newrem[r] = k - excl;
      }
    }
    __syncthreads();
  }
  if (t < nranks) s_np[t] = (K)(s_prefix[s_group[t]] | (K)((K)s_digit[t] << shift));
  __syncthreads();
  // regroup: a rank's leader is the first rank with its new prefix; groups are numbered in leader order
  if (t < nranks) {
    int leader = t;
    for (int r = t - 1; r >= 0; --r)
      if (s_np[r] == s_np[t]) leader = r;
    s_leader[t] = leader;
  }
  __syncthreads();
  if (t < nranks) {
    int g = 0;
    for (int r = 0; r < s_leader[t]; ++r) g += s_leader[r] == r ? 1 : 0;
    ws->group[t] = (unsigned)g;
    ws->rem[t] = s_newrem[t];
    if (s_leader[t] == t) ws->prefix[g] = (unsigned long long)s_np[t];
    if (pass == kPasses - 1) out[t] = bits_to_double(from_key<K>(s_np[t]));
  }
  if (t == 0) {
    int groups = 0;
    for (int r = 0; r < nranks; ++r) groups += s_leader[r] == r ? 1 : 0;
    ws->ngroups = (unsigned)groups;
    if (pass == kPasses - 1) {
      out[nranks] = (double)load_agent(&ws->nan);
      publish(&ws->nan, 0ull);
    }
    rearm(ws->ticket);
  }
}

template <typename K>
int launch_select(const void* x, int64_t n, const Ranks& ranks, int nranks, double* out, SelectWs* ws, hipStream_t q) {
  const unsigned g = grid_for<K>(n);
  const int64_t head = head_elements<K>(x, n);
  return dispatch_flag(stream_nt(n * (int64_t)sizeof(K)), [&](auto nt) {
    for (int pass = 0; pass < (int)sizeof(K); ++pass) {
      select_pass<K, decltype(nt)::value><<<g, kBlock, 0, q>>>((const K*)x, n, head, pass, nranks, ranks, ws, out);
      if (launch_status() != kOk) return (int)kLaunchFailed;
    }
    return (int)kOk;
  });
}

// ---- histogram ----------------------------------------------------------------------
// Edges (f64) and the block's u32 counts sit in dynamic LDS.  The bin of v is
// the last i with edges[i] <= v (the last bin closed on the right): a scaled
// estimate checked against the edges and moved by one bin if needed, else a
// binary search -- the edges decide, never how (v - e0) * scale rounds.  The
// index is clamped to [0, bins) whatever the edges hold.
struct HistWs {
  unsigned long long table[kMaxBins];  // merged counts; zero between launches
  alignas(256) unsigned ticket[64];
};

template <typename K, bool NT>
__global__ __launch_bounds__(kBlock) void histogram_kernel(const K* __restrict__ x, int64_t n, int64_t head,
                                                           const double* __restrict__ edges, int bins,
                                                           HistWs* __restrict__ ws,
                                                           unsigned long long* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
  double* e = reinterpret_cast<double*>(dyn);                       // bins + 1
  unsigned* hist = reinterpret_cast<unsigned*>(e + (bins + 1));     // bins
  for (int i = threadIdx.x; i <= bins; i += kBlock) e[i] = edges[i];
  for (int i = threadIdx.x; i < bins; i += kBlock) hist[i] = 0;
  __syncthreads();
  const double e0 = e[0], elast = e[bins];
  const double width = elast - e0;
  const double scale = width > 0.0 ? (double)bins / width : 0.0;  // (inf width: 0, the search decides)

  for_each_element<K, NT>(x, n, head, [&](K u) {
    const double v = bits_to_double(u);
    const bool in = v >= e0 && v <= elast;  // NaN: false
    int b = 0;
    if (in) {
      const double est = (v - e0) * scale;
      b = est >= (double)bins ? bins - 1 : est >= 0.0 ? (int)est : 0;  // NaN: 0
      b = b < 0 ? 0 : b > bins - 1 ? bins - 1 : b;
      bool ok = e[b] <= v && (b == bins - 1 || v < e[b + 1]);
      if (!ok) {
        if (v < e[b]) {
          if (b > 0) {
            --b;
            ok = e[b] <= v;
          }
        } else if (b + 1 < bins) {
          ++b;
          ok = b == bins - 1 || v < e[b + 1];
        }
      }
      if (!ok) {
        // the number of edges <= v, less one
        int lo = 0, hi = bins + 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (e[mid] <= v) lo = mid + 1;
          else hi = mid;
        }
        b = lo - 1;
        b = b < 0 ? 0 : b > bins - 1 ? bins - 1 : b;
      }
    }
    lds_count(hist, (unsigned)b, in);
  });
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += kBlock) {
    const unsigned c = hist[i];
    if (c) __hip_atomic_fetch_add(&ws->table[i], (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!take_last_ticket(ws->ticket, gridDim.x)) return;
  for (int i = threadIdx.x; i < bins; i += kBlock) {
    counts[i] = load_agent(&ws->table[i]);
    publish(&ws->table[i], 0ull);
  }
  if (threadIdx.x == 0) rearm(ws->ticket);
}

template <typename K>
int launch_histogram(const void* x, int64_t n, const double* edges, int bins, unsigned long long* counts, HistWs* ws,
                     hipStream_t q) {
  const unsigned g = grid_for<K>(n);
  const int64_t head = head_elements<K>(x, n);
  const size_t lds = (size_t)(bins + 1) * sizeof(double) + (size_t)bins * sizeof(unsigned);
  return dispatch_flag(stream_nt(n * (int64_t)sizeof(K)), [&](auto nt) {
    histogram_kernel<K, decltype(nt)::value><<<g, kBlock, lds, q>>>((const K*)x, n, head, edges, bins, ws, counts);
    return launch_status();
  });
}

}  // namespace stats

// A fresh workspace reads zero everywhere (table, NaN count, ticket); every call leaves it so.
WsLayout select_ws_layout() { return {(int64_t)sizeof(stats::SelectWs), 0, (int64_t)sizeof(stats::SelectWs)}; }
WsLayout histogram_ws_layout() { return {(int64_t)sizeof(stats::HistWs), 0, (int64_t)sizeof(stats::HistWs)}; }

}  // namespace bk

using namespace bk;
using namespace bk::stats;

// (contracts of the entry points: beekern.h)
BK_API int bk_select(int dtype, const void* x, int64_t n, const int64_t* ranks, int nranks, void* out,
                     void* workspace, hipStream_t stream) {
  if (!x || !ranks || !out || !workspace || n <= 0 || nranks < 1 || nranks > kMaxRanks) return kBadArgument;
  if (dtype != kF32 && dtype != kF64 && dtype != kBF16) return kBadArgument;
  if ((uintptr_t)x % (uintptr_t)dtype_size(dtype) != 0) return kBadArgument;
  Ranks r;
  memset(&r, 0, sizeof(r));
  for (int i = 0; i < nranks; ++i) {
    if (ranks[i] < 0 || ranks[i] >= n) return kBadArgument;
    r.k[i] = ranks[i];
  }
  SelectWs* ws = (SelectWs*)workspace;
  switch (dtype) {
    case kF64: return launch_select<uint64_t>(x, n, r, nranks, (double*)out, ws, stream);
    case kF32: return launch_select<uint32_t>(x, n, r, nranks, (double*)out, ws, stream);
    default: return launch_select<uint16_t>(x, n, r, nranks, (double*)out, ws, stream);
  }
}

BK_API int bk_histogram_max_bins() { return kMaxBins; }

BK_API int bk_histogram(int dtype, const void* x, int64_t n, const void* edges, int bins, void* counts,
                        void* workspace, hipStream_t stream) {
  if (!x || !edges || !counts || !workspace || n < 0 || bins < 1 || bins > kMaxBins) return kBadArgument;
  if (dtype != kF32 && dtype != kF64 && dtype != kBF16) return kBadArgument;
  if ((uintptr_t)x % (uintptr_t)dtype_size(dtype) != 0 || (uintptr_t)edges % 8 != 0 || (uintptr_t)counts % 8 != 0)
    return kBadArgument;
  HistWs* ws = (HistWs*)workspace;
  const double* e = (const double*)edges;
  unsigned long long* c = (unsigned long long*)counts;
  switch (dtype) {
    case kF64: return launch_histogram<uint64_t>(x, n, e, bins, c, ws, stream);
    case kF32: return launch_histogram<uint32_t>(x, n, e, bins, c, ws, stream);
    default: return launch_histogram<uint16_t>(x, n, e, bins, c, ws, stream);
  }
}
