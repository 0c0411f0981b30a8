// The scalar reductions' ops and trees (reduce.hip), and the closing ("tail")
// reduction a producer kernel can carry: the reduction bk_reduce would run
// next over the values the producer has just written, done by the producer's
// last block instead of a launch of its own (reduce.hip's axis reductions,
// gemm_bf16.hip's skinny product).
#pragma once
#include "bk_common.hpp"
#include "bk_ticket.hpp"

namespace bk {

// kRedMaxAbsDiff: max |a - b| (two operands, like kRedDot) -- one pass where
// subtract + abs + max would be three (e.g. a row check against a reference)
enum ReduceOp : int { kRedSum = 0, kRedSquareSum, kRedAbsSum, kRedMax, kRedMin, kRedDot, kRedMaxAbsDiff, kRedCount };
template <int OP> constexpr bool kTwoOperands = OP == kRedDot || OP == kRedMaxAbsDiff;

template <int OP> __device__ __forceinline__ double red_init() {
  if constexpr (OP == kRedMax) return -INFINITY;
  else if constexpr (OP == kRedMaxAbsDiff) return 0.0;
  else if constexpr (OP == kRedMin) return INFINITY;
  else return 0.0;
}
template <int OP> __device__ __forceinline__ double red_map(double a, double b) {
  if constexpr (OP == kRedSquareSum) return a * a;
  else if constexpr (OP == kRedAbsSum) return fabs(a);
  else if constexpr (OP == kRedDot) return a * b;
  else if constexpr (OP == kRedMaxAbsDiff) return fabs(a - b);
  else return a;
}
// max / min propagate NaN as numpy's max() / min() do (fmax / fmin are IEEE
// maxNum: they drop a NaN operand, so a max-abs-difference check of a result
// holding NaN would return a finite "error")
template <int OP> __device__ __forceinline__ double red_combine(double x, double y) {
  if constexpr (OP == kRedMax || OP == kRedMaxAbsDiff) return (x != x || y != y) ? __builtin_nan("") : fmax(x, y);
  else if constexpr (OP == kRedMin) return (x != x || y != y) ? __builtin_nan("") : fmin(x, y);
  else return x + y;
}

template <int OP> __device__ __forceinline__ double wave_reduce(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = red_combine<OP>(v, __shfl_xor(v, off, kWave));
  return v;
}

// BLOCK: the threads of the calling block, all of which call.  Waves past the
// first kRedBlock / kWave that pass the op's identity leave the result what
// the kRedBlock tree gives (their partials are identities, as the padding
// lanes of its last step are).
template <int OP, int BLOCK = kRedBlock> __device__ __forceinline__ double block_reduce(double v) {
  constexpr int kWaves = BLOCK / kWave;
  __shared__ double partial[kWaves];
  v = wave_reduce<OP>(v);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) partial[wid] = v;
  __syncthreads();
  double r = red_init<OP>();
  if (wid == 0) {
    r = lane < kWaves ? partial[lane] : red_init<OP>();
    r = wave_reduce<OP>(r);
  }
  return r;
}

// ---- the closing reduction ------------------------------------------------------
// bk_reduce launches one block while n / (16 / sizeof(T)) <= kTailMaxVectors
// (launch_reduce in reduce.hip: four vectors per lane before a second block),
// whatever BK_REDUCE_BLOCKS says; only then is there a tail.  BK_TAIL_MAX_VECTORS
// of beekern.h is this number.
constexpr int64_t kTailMaxVectors = 4 * kRedBlock;
constexpr int kTailUnroll = 16;  // reduce.hip kRedUnroll: the accumulators of a reduce_1pass lane
static_assert(kTailMaxVectors == BK_TAIL_MAX_VECTORS, "beekern.h and bk_reduce_ops.hpp disagree on the tail limit");
template <typename T> inline bool tail_fits(int64_t n) { return n >= 0 && n / (int64_t)(16 / sizeof(T)) <= kTailMaxVectors; }

// what the producer's last block reduces, and where the scalar goes: a and b
// as bk_reduce takes them (one of them the producer's output), the ticket of
// the BK_WS_REDUCE workspace, bk_reduce's result slot
struct Tail {
  const void* a;
  const void* b;
  int64_t n;
  unsigned* ticket;
  double* out;
};

// the lab layouts of bk_reduce (BK_REDUCE_LAYOUT) add in another order than the tail does
inline bool reduce_lab_layout() {
  static const bool lab = getenv("BK_REDUCE_LAYOUT") && getenv("BK_REDUCE_LAYOUT")[0] != '\0';
  return lab;
}
// The tail descriptor of an entry point's arguments; false where there is no
// tail for them (the caller then launches the producer and bk_reduce):
// `produced` is the producer's output, `count` elements of T; one of a and b,
// which bk_reduce's op reads, must be it.
template <typename T>
bool make_tail(int tail_op, const void* a, const void* b, int64_t n, void* tail_ws, void* tail_out, const void* produced,
               int64_t count, Tail* t) {
  if (tail_op < 0 || tail_op >= kRedCount || !a || !tail_ws || !tail_out || n != count || !tail_fits<T>(n)) return false;
  const bool two = tail_op == kRedDot || tail_op == kRedMaxAbsDiff;
  if (two ? (!b || (a != produced && b != produced)) : a != produced) return false;
  if (reduce_lab_layout()) return false;
  *t = Tail{a, two ? b : nullptr, n, reinterpret_cast<unsigned*>((double*)tail_ws + kRedMaxBlocks), (double*)tail_out};
  return true;
}

// Called by every thread of a producer block once the block's stores are
// issued; `blocks` such calls are made per launch.  The producer's stores are
// agent-scope (publish) and complete before the ticket (take_last_ticket);
// the last block reads both operands through load_agent -- the other XCDs' L2s
// are not this one's -- and adds them in the order the one-block reduce_1pass
// does: the lane's vectors t, t + 256, t + 512, t + 768 in four accumulators
// when it has all four, else one accumulator; the scalar rest; the sixteen
// accumulators left to right; block_reduce; then the fold of that single
// partial (identity first, seven identities after) and block_reduce again.
// The result has bk_reduce's bits.
template <typename T, int OP, int BLOCK>
__device__ __forceinline__ void run_tail(const Tail& t, unsigned blocks) {
  if (!take_last_ticket(t.ticket, blocks)) return;
  constexpr int N = 16 / sizeof(T);
  constexpr int U = kTailUnroll, U2 = 4, F = 8;  // reduce_1pass's accumulators, its second loop's and the fold's loads in flight
  const T* a = static_cast<const T*>(t.a);
  const T* b = static_cast<const T*>(t.b);
  const int64_t n = t.n, nvec = n / N;
  const int64_t stride = kRedBlock, tid = threadIdx.x;
  double acc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) acc[u] = red_init<OP>();
  const auto take = [&](double& r, int64_t k) {
    const double bk_ = kTwoOperands<OP> ? widen<T>(load_agent(b + k)) : 0.0;
    r = red_combine<OP>(r, red_map<OP>(widen<T>(load_agent(a + k)), bk_));
  };
  if (tid < kRedBlock) {  // (the lanes of bk_reduce's block)
    int64_t i = tid;
    for (; i + (U2 - 1) * stride < nvec; i += U2 * stride)
#pragma unroll
      for (int u = 0; u < U2; ++u)
#pragma unroll
        for (int j = 0; j < N; ++j) take(acc[u], (i + u * stride) * N + j);
    for (; i < nvec; i += stride)
#pragma unroll
      for (int j = 0; j < N; ++j) take(acc[0], i * N + j);
    for (int64_t k = nvec * N + tid; k < n; k += stride) take(acc[0], k);
  }
  double v = acc[0];
#pragma unroll
  for (int u = 1; u < U; ++u) v = red_combine<OP>(v, acc[u]);
  const double partial = block_reduce<OP, BLOCK>(v);
  __syncthreads();  // block_reduce's LDS is written again below
  double r = red_init<OP>();
  if (threadIdx.x == 0) {
    r = red_combine<OP>(r, partial);
#pragma unroll
    for (int u = 1; u < F; ++u) r = red_combine<OP>(r, red_init<OP>());
  }
  r = block_reduce<OP, BLOCK>(r);
  if (threadIdx.x == 0) {
    *t.out = r;
    rearm(t.ticket);
  }
}

// How a producer stores an output element, and what it does once its stores
// are issued.  Plain: a store, nothing after.
struct PlainOut {
  static constexpr bool kTail = false;
  template <typename TO> __device__ __forceinline__ void store(TO* out, int64_t i, TO v) const { out[i] = v; }
};
// a second, converted output: cast_out[i] is what bk_cast makes of out[i]
// (elementwise.hip cast_kernel: f64 -> bf16 through f32, everything else one conversion)
template <typename TO, typename TC> __device__ __forceinline__ TC cast_elem(TO v) {
  if constexpr (std::is_same<TC, uint16_t>::value) {
    if constexpr (std::is_same<TO, double>::value) return double_to_bf16_bits(v);
    else return float_to_bf16_bits(v);
  } else {
    return (TC)v;
  }
}
template <typename TC>
struct CastOut {
  static constexpr bool kTail = false;
  TC* cast_out;
  template <typename TO> __device__ __forceinline__ void store(TO* out, int64_t i, TO v) const {
    out[i] = v;
    cast_out[i] = cast_elem<TO, TC>(v);
  }
};
// the tail attached: agent-scope stores (the last block may sit on another XCD)
template <int OP>
struct TailOut {
  static constexpr bool kTail = true;
  static constexpr int kOp = OP;
  Tail tail;
  template <typename TO> __device__ __forceinline__ void store(TO* out, int64_t i, TO v) const { publish(out + i, v); }
};

}  // namespace bk
