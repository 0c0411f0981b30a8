// The C interface of libbeekern.so, declared once.
//
// Every kernel translation unit and runtime.cpp include this header (through
// bk_common.hpp), so a definition whose types differ from its declaration does
// not compile; the kernel broker (csrc/executor/broker.cpp) types its dlsym'd
// pointers as decltype(&bk_name); ops/_native.py's SIGNATURES table is checked
// against it by tests/test_native_abi_cpu.py.  Plain C++ can include it:
// nothing here needs hipcc.
//
// Each declaration starts with BK_API at the beginning of a line and ends at
// the first `;` (the test reads them that way).
//
// Conventions: every entry point takes raw device pointers and a hipStream_t,
// returns a status code (0 ok, 1 bad argument, 2 launch failed, 3 out of device
// memory, 4 quota exceeded, 5 not initialised: bk::Status of bk_common.hpp)
// unless said otherwise, and -- the allocator and the synchronous copies aside
// -- never allocates or synchronises.  dtype codes: 0 f32, 1 f64, 2 bf16,
// 3 f16, 4 i32, 5 i64, 6 bool (bk::DType).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime_api.h>

#define BK_API extern "C" __attribute__((visibility("default")))

// ---- limits --------------------------------------------------------------------
// (csrc/executor/broker_core.hpp keeps HIP-free copies of the first two,
// ops/driver.py and ops/array.py the Python side's; broker.cpp and
// tests/test_native_abi_cpu.py check them against these)
enum {
  BK_MAX_RANKS = 32,                // ranks per bk_select call
  BK_MAX_BINS = 4096,               // bins per bk_histogram call
  BK_MAX_AXIS0_COLUMNS = 1 << 18,   // columns bk_reduce_axis / bk_axis_stat reduce along axis 0
  BK_TAIL_MAX_VECTORS = 1024,       // 16-B vectors of a closing reduction's operand (bk_reduce_axis_tail)
  BK_MAX_SORT_N = 0x7fffffff,       // elements per bk_sort call (it carries 32-bit indices)
};

// ---- ticketed scratch workspaces -------------------------------------------------
// Device memory a kernel family keeps between launches: partials, tables and
// the completion tickets (bk_ticket.hpp).  One per stream of launches; a fresh
// one must be initialised once (its tickets, and the tables that are "zero
// between launches", must read zero -- every launch leaves them so).
enum BkWorkspace {
  BK_WS_REDUCE = 0,    // bk_reduce, bk_rand_reduce, bk_compare_count, bk_int_reduce, bk_arg_reduce, bk_take
  BK_WS_REDUCE_AXIS,   // bk_reduce_axis
  BK_WS_AXIS_STAT,     // bk_axis_stat
  BK_WS_COMPRESS,      // bk_compress
  BK_WS_SELECT,        // bk_select
  BK_WS_HISTOGRAM,     // bk_histogram
  BK_WS_COUNT
};
// the size of a workspace of `kind`; 0 for an unknown kind.  Pure host code.
BK_API int64_t bk_workspace_bytes(int kind);
// queues the zeroing of a fresh workspace on `stream`, ahead of its first
// launch there.  kBadArgument for an unknown kind or a null workspace, before
// any HIP call.
BK_API int bk_workspace_init(int kind, void* ws, hipStream_t stream);

// ---- runtime (runtime.cpp) ---------------------------------------------------------
// the calling thread's last error text (never null)
BK_API const char* bk_last_error();
BK_API int bk_version();
// Select the device, create the context and load this code object so the
// first user kernel launch pays nothing (measured: ~60-480 ms hipInit and
// ~90-140 ms first-launch module load on MI355X, paid while the sandbox
// waits in the warm pool instead of on the request path).
BK_API int bk_init(int device);
// the device of bk_init, -1 before it
BK_API int bk_device();
// the HBM quota of bk_malloc in bytes; 0 (or less): unlimited
BK_API int bk_set_quota(int64_t bytes);
BK_API int64_t bk_quota();
BK_API int bk_malloc(void** out, int64_t nbytes);
BK_API int bk_free(void* p);
// cached blocks and idle segments back to the driver
BK_API int bk_empty_cache();
// Serve large blocks from segments from now on, and reserve one of `bytes`
// now (the kernel broker at start-up): the first requests' large
// allocations are carved from it.
BK_API int bk_reserve(int64_t bytes);
// stats[0]=in_use, [1]=cached (small-block cache + free segment bytes), [2]=peak, [3]=quota
BK_API int bk_memory_stats(int64_t* stats);
// kind: 1 = H2D, 2 = D2H, 3 = D2D (hipMemcpyKind values); synchronous on `stream`
BK_API int bk_memcpy(void* dst, const void* src, int64_t nbytes, int kind, hipStream_t stream);
BK_API int bk_memcpy_async(void* dst, const void* src, int64_t nbytes, int kind, hipStream_t stream);
BK_API int bk_sync(hipStream_t stream);
// Run one tiny launch from every kernel module so HIP loads the code objects
// now: with deferred loading the first launch from each module costs tens of
// ms (measured in the served path: the first bk.rand 128 ms, the first
// rand_reduce 34 ms; profiles/archive/r1_served_path_final_ranges.csv), which a
// long-lived process (the kernel broker) should pay at startup, not on a
// request.  Returns the first failure.
BK_API int bk_preload(hipStream_t stream);
// info[0]=CUs, [1]=total bytes, [2]=free bytes, [3]=clock kHz, [4]=LDS/CU bytes
BK_API int bk_device_info(int64_t* info, char* name, int name_len);
// Timing helper for benches: elapsed ms between two events recorded on stream.
BK_API int bk_event_pair_create(void** start, void** stop);
BK_API int bk_event_record(void* ev, hipStream_t stream);
BK_API float bk_event_elapsed_ms(void* start, void* stop);
BK_API int bk_event_destroy(void* ev);

// ---- random draws (random.hip) -------------------------------------------------------
// dtype: kF64, kF32 or kBF16 (the f32 stream, rounded).  `offset` advances the counter so successive draws from
// one seed never overlap (the Python side keeps the running offset).
BK_API int bk_rand_uniform(void* out, int64_t n, int dtype, uint64_t seed, uint64_t offset, double lo, double hi,
                           hipStream_t stream);
BK_API int bk_rand_normal(void* out, int64_t n, int dtype, uint64_t seed, uint64_t offset, double mean, double std,
                          hipStream_t stream);
// the continuous distributions of bk_rand_dist and what p0, p1 mean for each (an unused one is passed as 0)
enum BkRandDist {
  BK_DIST_EXPONENTIAL = 0,  // p0 scale
  BK_DIST_LAPLACE,          // p0 loc, p1 scale
  BK_DIST_LOGISTIC,         // p0 loc, p1 scale
  BK_DIST_GUMBEL,           // p0 loc, p1 scale
  BK_DIST_RAYLEIGH,         // p0 scale
  BK_DIST_WEIBULL,          // p0 a
  BK_DIST_PARETO,           // p0 a (numpy's Lomax form)
  BK_DIST_CAUCHY,           // p0 loc, p1 scale
  BK_DIST_LOGNORMAL,        // p0 mean, p1 sigma of the underlying normal
  BK_DIST_GAMMA,            // p0 shape, p1 scale
  BK_DIST_BETA,             // p0 a, p1 b
  BK_DIST_STUDENT_T,        // p0 df
  BK_DIST_COUNT
};
// n draws of `kind` at (seed, offset); dtype kF64 or kF32.  Kinds 0-7 are one transform of an open-interval
// uniform and consume a counter per 2 f64 / 4 f32 elements, as bk_rand_uniform (streams of their own); lognormal
// is exp of bk_rand_normal's value for the same (seed, offset, mean, sigma); gamma, beta and student t are
// rejection samplers in f64 (the f32 result is the f64 value rounded once) that consume one counter per element:
// element i depends on (seed, offset + i) alone.  No value is inf or NaN for exponential .. cauchy, lognormal
// within exp's range.  kBadArgument before any launch for an unknown kind, another dtype, a null out, n < 0, a
// non-finite p0 or p1, or a parameter outside its domain (scale, sigma >= 0; shape, a, b, df > 0); n = 0 is kOk.
BK_API int bk_rand_dist(int kind, void* out, int64_t n, int dtype, uint64_t seed, uint64_t offset, double p0, double p1,
                        hipStream_t stream);

// ---- elementwise (elementwise.hip) ------------------------------------------------------
// f64 computes in f64; f32 and bf16 compute in f32 (bf16 rounds once on store).
// abs clears the sign bit: abs(-0.0) = +0.0 and a NaN comes out positive, as numpy.absolute.
// relu is numpy.maximum(x, 0): NaN in gives NaN out; both zeros and every negative give +0.0.
BK_API int bk_unary(int op, int dtype, const void* x, void* y, int64_t n, hipStream_t stream);
// mode: 0 = array (op) array, 1 = array (op) scalar, 2 = scalar (op) array.
// The scalar is converted once to the compute type (f64; f32 for f32 and bf16
// arrays) and the arithmetic runs there: x + 0.1 on f32 adds float(0.1), as
// numpy does for a Python scalar.
BK_API int bk_binary(int op, int dtype, int mode, const void* a, const void* b, double scalar, void* y, int64_t n,
                     hipStream_t stream);
BK_API int bk_cast(int src_dtype, int dst_dtype, const void* x, void* y, int64_t n, hipStream_t stream);
BK_API int bk_fill(void* y, int64_t nbytes, uint64_t pattern, int pattern_bytes, hipStream_t stream);

// ---- reductions (reduce.hip) -------------------------------------------------------------
// out: ONE double on the device.  workspace: BK_WS_REDUCE.
// b is only read for kRedDot and kRedMaxAbsDiff (same length and dtype as a).
// Every result is an f64 accumulation of the input widened to f64 (exactly, for
// f32 and bf16): the square of f32 3e38 is the finite f64 value, not inf.
// n = 0 (a, and b where it is read, still valid pointers) is kOk and stores the
// op's identity: 0.0 for sum, square_sum, abs_sum and dot, -inf for max, +inf
// for min, 0.0 for max_abs_diff; the workspace is left ready for the next launch.
BK_API int bk_reduce(int op, int dtype, const void* a, const void* b, int64_t n, void* workspace, void* out,
                     hipStream_t stream);
// sum (op 0) or square-sum (op 1) of the uniform [lo, hi) draw of n values
// at (seed, offset) -- without materialising it.  dtype kF64 or kF32.
BK_API int bk_rand_reduce(int op, int dtype, int64_t n, uint64_t seed, uint64_t offset, double lo, double hi,
                          void* workspace, void* out, hipStream_t stream);
// out[cols] (axis 0) or out[rows] (axis 1) = sum (op 0) or mean (op 1) of
// x[rows x cols] (row stride ld).  out dtype: f64 for f64 input, f32 for f32
// and bf16 input (f64 accumulation throughout).  ws: BK_WS_REDUCE_AXIS.
BK_API int bk_reduce_axis(int op, int dtype, const void* x, int64_t rows, int64_t cols, int64_t ld, int axis, void* out,
                          void* ws, hipStream_t stream);
// bk_reduce_axis, and cast_out[i] = out[i] converted to cast_dtype (kF32, kF64
// or kBF16, another dtype than out's) exactly as bk_cast converts it: the bits
// of bk_reduce_axis followed by bk_cast, in one launch.  out is written too.
// cast_out is another buffer than out and x.
BK_API int bk_reduce_axis_cast(int op, int dtype, const void* x, int64_t rows, int64_t cols, int64_t ld, int axis,
                               void* out, int cast_dtype, void* cast_out, void* ws, hipStream_t stream);
// bk_reduce_axis, and then what bk_reduce(tail_op, out's dtype, tail_a, tail_b,
// tail_n, tail_ws, tail_out) would store, in one launch: the last block to
// finish reduces.  One of tail_a and tail_b (tail_a for a one-operand op) is
// `out`, the other a buffer no part of this launch writes; tail_n is the
// number of elements out gets and spans at most BK_TAIL_MAX_VECTORS 16-byte
// vectors (where bk_reduce runs a single block: the scalar then has its
// bits); tail_ws: BK_WS_REDUCE.  kBadArgument, with nothing launched, where
// there is no such tail: launch bk_reduce_axis and bk_reduce instead.
BK_API int bk_reduce_axis_tail(int op, int dtype, const void* x, int64_t rows, int64_t cols, int64_t ld, int axis,
                               void* out, void* ws, int tail_op, const void* tail_a, const void* tail_b, int64_t tail_n,
                               void* tail_ws, void* tail_out, hipStream_t stream);

// ---- int64 arrays (integer.hip) ---------------------------------------------------------
// Every array element is an int64_t; a pointer need only be 8-byte aligned.
// op: 0 add, 1 subtract, 2 multiply, 3 floor_divide, 4 remainder, 5 maximum, 6 minimum; mode as bk_binary.
// add, subtract and multiply wrap in two's complement; floor_divide and remainder follow Python's sign rule
// (floor; the remainder takes the divisor's sign), give 0 for a zero divisor, and INT64_MIN // -1 = INT64_MIN,
// INT64_MIN % -1 = 0 (numpy's answers on x86-64).  y may be a or b.
BK_API int bk_int_binary(int op, int mode, const void* a, const void* b, int64_t scalar, void* y, int64_t n,
                         hipStream_t stream);
// op: the codes of bk_compare; mode 0 = array (op) array, 1 = array (op) scalar; mask_out: n bytes of 0 / 1
BK_API int bk_int_compare(int op, int mode, const void* a, const void* b, int64_t scalar, void* mask_out, int64_t n,
                          hipStream_t stream);
// op: 0 sum (wrapping), 1 max, 2 min.  out: ONE int64 on the device.  workspace: BK_WS_REDUCE.  One launch; exact
// and independent of the grid.  n = 0 (a still a valid pointer) is kOk and stores 0 / INT64_MIN / INT64_MAX; the
// workspace is left ready for the next launch.
BK_API int bk_int_reduce(int op, const void* a, int64_t n, void* workspace, void* out, hipStream_t stream);
// exactly kI64 -> kF64, kI64 -> kF32 (round to nearest even), kF64 -> kI64, kF32 -> kI64, kBool -> kI64 (any
// non-zero byte -> 1); another pair is kBadArgument.  Float to int truncates toward zero; NaN, +-inf and anything
// outside [-2^63, 2^63) give INT64_MIN (numpy's astype on x86-64).
BK_API int bk_int_cast(int src_dtype, int dst_dtype, const void* x, void* y, int64_t n, hipStream_t stream);
// the integer-valued draws of bk_rand_int and what a, b, p mean for each (an unused one is passed as 0)
enum BkRandInt {
  BK_RINT_INTEGERS = 0,  // a low, b high (exclusive), b > a
  BK_RINT_POISSON,       // p lam, 0 <= lam <= 2^53
  BK_RINT_BINOMIAL,      // a trials, 0 <= trials < 2^53; p in [0, 1]
  BK_RINT_GEOMETRIC,     // p in (0, 1]
  BK_RINT_COUNT
};
// n int64 draws of `kind` at (seed, offset): element i depends on (seed, offset, i) and the parameters alone.
// integers consume a counter per 4 elements (span b - a <= 2^32: Lemire's multiply-shift on one word) or per 2
// (wider spans: on a 64-bit word); geometric one per 2; poisson (multiplication method below lam 10, Hoermann's
// PTRS from there) and binomial (inversion below trials * min(p, 1 - p) = 10, Hoermann's BTRS from there) one per
// element.  Every rejection loop ends after 64 Philox calls with the current candidate, clamped into the support.
// kBadArgument before any launch for an unknown kind, a null out, n < 0 or a parameter outside its domain; n = 0
// is kOk.
BK_API int bk_rand_int(int kind, void* out, int64_t n, uint64_t seed, uint64_t offset, int64_t a, int64_t b, double p,
                       hipStream_t stream);

// ---- boolean masks (mask.hip): one byte per element ------------------------------------------
// mode: 0 = array (op) array, 1 = array (op) scalar; mask_out: n bytes of 0 / 1
BK_API int bk_compare(int op, int dtype, int mode, const void* a, const void* b, double scalar, void* mask_out,
                      int64_t n, hipStream_t stream);
// the number of true comparisons as ONE double in *out, no mask written.
// workspace: BK_WS_REDUCE (the reductions' own).
BK_API int bk_compare_count(int op, int dtype, int mode, const void* a, const void* b, double scalar, int64_t n,
                            void* workspace, void* out, hipStream_t stream);
// op: 0 and, 1 or, 2 xor, 3 not (b unused); inputs normalised with != 0
BK_API int bk_mask_logical(int op, const void* a, const void* b, void* out, int64_t n, hipStream_t stream);
// out[i] = mask[i] ? A : B; flags bit 0: A is the scalar sa, bit 1: B is the
// scalar sb.  Scalars are converted to the dtype once (f32: RNE; bf16: f32
// then RNE); array values move as bits.
BK_API int bk_where(int dtype, const void* mask, int flags, const void* a, const void* b, double sa, double sb,
                    void* out, int64_t n, hipStream_t stream);
// out[0 : min(count, cap)] = x[mask] in index order (two launches); dtype:
// f32 / f64 / bf16 / bool, moved by size.  A write at index >= cap is dropped.
// workspace: BK_WS_COMPRESS.
BK_API int bk_compress(int dtype, const void* x, const void* mask, int64_t n, void* out, int64_t cap, void* workspace,
                       hipStream_t stream);

// ---- order statistics and histograms (stats.hip) -----------------------------------------------
// out[i] = np.sort(x)[ranks[i]] widened to f64 for the nranks (1..BK_MAX_RANKS)
// 0-based ranks, each in [0, n); out[nranks] = the number of NaNs in x (they
// sort last).  `ranks` is read on the host during the call; x, out and the
// workspace (BK_WS_SELECT) are device memory.
// One launch per byte of the dtype; x is only read.
BK_API int bk_select(int dtype, const void* x, int64_t n, const int64_t* ranks, int nranks, void* out,
                     void* workspace, hipStream_t stream);
// BK_MAX_BINS
BK_API int bk_histogram_max_bins();
// counts[i] (u64, i < bins) = the number of elements v of x, widened to f64,
// with edges[i] <= v < edges[i + 1] (the last bin also takes v ==
// edges[bins]): np.histogram's rule.  edges: bins + 1 non-decreasing f64 in
// device memory, 1 <= bins <= BK_MAX_BINS.  NaNs and values outside the edges
// count nowhere; what counts held before does not matter.  One launch.
// workspace: BK_WS_HISTOGRAM.
BK_API int bk_histogram(int dtype, const void* x, int64_t n, const void* edges, int bins, void* counts,
                        void* workspace, hipStream_t stream);

// ---- sorting, arg-reductions and gather (sort.hip) ---------------------------------------------
// The order is numpy's: floats numerically with -0.0 == +0.0 a tie and every NaN, of either sign, tied last;
// int64 signed; ties keep index order.
// the bytes of bk_sort's `ws` (a caller-sized data buffer, as bk_gemm_f32x6's, not a ticketed workspace); 0 for an
// unknown dtype, n < 0 or n > BK_MAX_SORT_N.  Pure host code.
BK_API int64_t bk_sort_workspace_bytes(int dtype, int64_t n, int with_index);
// sorted_out[0:n) = np.sort(x) (the sign of a zero among zeros and a NaN's payload aside), index_out[0:n) (int64) =
// np.argsort(x, kind="stable"); either may be null, not both.  dtype kF32, kF64, kBF16 or kI64; x is only read;
// x, the outputs and ws (16-byte aligned, ws_bytes >= bk_sort_workspace_bytes(dtype, n, index_out != null)) do not
// overlap.  An LSD radix sort: two launches per byte of the dtype.  n = 0 is kOk with nothing launched.
BK_API int bk_sort(int dtype, const void* x, int64_t n, void* sorted_out, void* index_out, void* ws, int64_t ws_bytes,
                   hipStream_t stream);
// op 0 argmax, 1 argmin: ONE int64 in *out, numpy's answer (the first occurrence; the first NaN if x holds one).
// dtype kF32, kF64, kBF16 or kI64.  n < 1 is kBadArgument.  workspace: BK_WS_REDUCE.  One launch.
BK_API int bk_arg_reduce(int op, int dtype, const void* x, int64_t n, void* workspace, void* out, hipStream_t stream);
// out[i] = x[idx[i]] for m int64 indices, each in [-n, n) (negative: from the end); elements move by size (f32,
// f64, bf16, bool, i64).  An index outside that range is never dereferenced: its out element gets zero bits and it
// is counted.  *bad_out: ONE int64, the number of such indices.  workspace: BK_WS_REDUCE.  One launch (m = 0 too).
BK_API int bk_take(int dtype, const void* x, int64_t n, const void* idx, int64_t m, void* out, void* workspace,
                   void* bad_out, hipStream_t stream);

// ---- a matrix against a vector, per-axis statistics (axis.hip) ------------------------------------
// y[rows x cols] (row stride ldy) = a[rows x cols] (row stride lda) OP v, with
// v[cols] along the rows (kind 0) or v[rows] down the columns (kind 1);
// swapped: v OP a.  op: the codes of bk_binary.  f32 / f64.  y may be a
// itself (same pointer and stride); any other overlap of y with a or v is
// refused.
BK_API int bk_broadcast(int op, int dtype, int kind, int swapped, const void* a, int64_t rows, int64_t cols, int64_t lda,
                        const void* v, void* y, int64_t ldy, hipStream_t stream);
// out[cols] (axis 0) or out[rows] (axis 1) = max (op 0), min (1), variance (2)
// or standard deviation (3) of x[rows x cols] (row stride ld), in x's dtype
// (f32 / f64; f64 arithmetic throughout).  divisor: n - ddof of the variance
// (finite, > 0; unused by max / min).  ws: BK_WS_AXIS_STAT.
BK_API int bk_axis_stat(int op, int dtype, const void* x, int64_t rows, int64_t cols, int64_t ld, int axis,
                        double divisor, void* out, void* ws, hipStream_t stream);

// ---- bf16 GEMM and transposes (gemm_bf16.hip) --------------------------------------------------------
// 1 if the 128x128 kernel takes the shape (tile multiples, ld multiples of 8)
BK_API int bk_gemm_bf16_fast_ok(int M, int N, int K, int lda, int ldb);
// C = alpha * A . Bt^T + beta * C.  out_dtype: kBF16 or kF32.
BK_API int bk_gemm_bf16_tn(const void* A, const void* Bt, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                           float alpha, float beta, int out_dtype, hipStream_t stream);
// the same with the kernel named: variant 0 = auto, 1 = generic, 2 = 128x128,
// 3 = 256x256 (4-wave or 8-wave by K), 4 = 256x256 8-wave, 5 = 256x256 4-wave,
// 6 = 128x128 edge, 7 = 256x256 4-wave edge, 8 = skinny (N <= 16: a
// matrix-vector product) (benchmarks, tests).  kBadArgument if the named
// kernel cannot take the operands.
BK_API int bk_gemm_bf16_tn_variant(const void* A, const void* Bt, void* C, int M, int N, int K, int lda, int ldb,
                                   int ldc, float alpha, float beta, int out_dtype, int variant, hipStream_t stream);
// The skinny product (N <= 16, what variant 0 picks for such operands) with
// beta == 0 and ldc == N, and then bk_reduce(tail_op, out_dtype, tail_a,
// tail_b, tail_n = M * N, tail_ws, tail_out) in the same launch: the rules of
// bk_reduce_axis_tail, with C as the produced buffer.  kBadArgument, with
// nothing launched, for any other product or tail.
BK_API int bk_gemm_bf16_tn_tail(const void* A, const void* Bt, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                                float alpha, float beta, int out_dtype, int tail_op, const void* tail_a,
                                const void* tail_b, int64_t tail_n, void* tail_ws, void* tail_out, hipStream_t stream);
// Which kernel `variant 0` resolves to for these operands (diagnostics).
BK_API int bk_gemm_bf16_pick(const void* A, const void* Bt, const void* C, int M, int N, int K, int lda, int ldb,
                             int ldc, int out_dtype);
// C = alpha * A . B + beta * C with B stored [K][N] (leading dimension ldb):
// the 4-wave 256x256 kernel reading B through transposed LDS reads, no
// transpose pass.  Tile-multiple shapes (M, N % 256, K % 64) with 16-B
// aligned operands only: kBadArgument otherwise (callers transpose B and use
// bk_gemm_bf16_tn).  bk_gemm_bf16_nn_ok: 1 if bk_gemm_bf16_nn takes them.
BK_API int bk_gemm_bf16_nn_ok(const void* A, const void* B, const void* C, int M, int N, int K, int lda, int ldb,
                              int ldc, int out_dtype);
BK_API int bk_gemm_bf16_nn(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                           float alpha, float beta, int out_dtype, hipStream_t stream);
// out[cols x rows] = transpose of in[rows x cols], bf16
BK_API int bk_transpose_bf16(const void* in, void* out, int rows, int cols, int ld_in, int ld_out,
                             hipStream_t stream);
// out[cols x rows] (bf16) = transpose of in[rows x cols] (src_dtype kBF16,
// kF32 or kF64).  Wide inputs need the 8-aligned, 16-B aligned shape of the
// vector kernel (kBadArgument otherwise: the caller casts, then transposes).
BK_API int bk_transpose_to_bf16(int src_dtype, const void* in, void* out, int rows, int cols, int ld_in, int ld_out,
                                hipStream_t stream);
// out[cols x rows] = transpose of in[rows x cols].  dst_dtype kBF16 converts
// (bk_transpose_to_bf16); dst_dtype == src_dtype moves the bits (2-, 4- or
// 8-byte elements).
BK_API int bk_transpose(int src_dtype, int dst_dtype, const void* in, void* out, int rows, int cols, int ld_in,
                        int ld_out, hipStream_t stream);

// ---- f64 / f32 GEMM (gemm_fp.hip) -------------------------------------------------------------------------
// C[M][N] = op(A) . op(B) in f64 (dtype kF64) or f32 (kF32), row-major C with
// leading dimension ldc.  trans_a: A is given as its transpose, a [K][M]
// buffer (lda >= M); else [M][K] (lda >= K).  trans_b: B given as a [N][K]
// buffer (ldb >= K); else [K][N] (ldb >= N).  Never reads C.
BK_API int bk_gemm_fp(int dtype, int trans_a, int trans_b, const void* A, const void* B, void* C, int M, int N, int K,
                      int64_t lda, int64_t ldb, int64_t ldc, hipStream_t stream);
// the bytes of bk_gemm_f32x6's `ws` for the shape (a caller-sized data buffer,
// not a ticketed workspace); 0 for a non-positive dimension
BK_API int64_t bk_gemm_f32x6_workspace_bytes(int M, int N, int K);
// C = op(A) . op(B) for f32 operands on the bf16 MFMA GEMM, f32-level error
// (the six-piece split of gemm_fp.hip).  Same operand conventions as
// bk_gemm_fp.  `ws` (16-B aligned, bk_gemm_f32x6_workspace_bytes) holds a
// flag word and the split operands A' [M][6 Kp], B' [N][6 Kp].  Operands the
// split cannot represent (inf / NaN, |x| >= 2^127, 0 < |x| < 2^-100) make the
// plain f32 kernel recompute C, gated on the flag (no host sync).
BK_API int bk_gemm_f32x6(int trans_a, int trans_b, const void* A, const void* B, void* C, int M, int N, int K,
                         int64_t lda, int64_t ldb, int64_t ldc, void* ws, int64_t ws_bytes, hipStream_t stream);
