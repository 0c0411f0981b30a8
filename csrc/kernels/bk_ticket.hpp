// Single-launch completion tickets and the grid and workspace numbers that go
// with them, shared by the reductions (reduce.hip), the mask kernels
// (mask.hip) and the axis statistics (axis.hip); stats.hip takes the tickets.
//
// Every block publishes its partial, then takes a ticket; the block holding
// the last ticket folds the partials and re-arms the ticket for the next
// launch on this workspace.  Tickets start at zero (bk_workspace_init).
// No block ever waits for another: the last one to arrive does the fold.
//
// Blocks sit on different XCDs, each with its own L2.  Partials are written
// and read with agent-scope (sc1) accesses, which are coherent across XCDs;
// a store is complete (vmcnt: GFX9 counts stores there) before its block's
// ticket.  No release/acquire fences: at agent scope those write back and
// invalidate the whole L2 (buffer_wbl2 / buffer_inv), per block -- what the
// first version of this did cost every reduction ~1 ms under concurrent
// sandboxes.
#pragma once
#include "bk_common.hpp"

// The fold relies on GFX9-family memory semantics: vmcnt counts stores and
// sc1 (agent-scope) accesses are coherent across XCDs.  gfx10+ counts stores
// in vscnt, so the fold could read partials that have not landed -- refuse to
// build for anything but gfx9 (gfx950 here).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "bk_ticket.hpp: the single-pass ticket fold is written for GFX9-family (gfx950) memory semantics"
#endif

namespace bk {

constexpr int kRedBlock = 256;
// the reduction workspace holds kRedMaxBlocks f64 partials, then the ticket
// (its own 256 B): BK_WS_REDUCE
constexpr int kRedMaxBlocks = 32768;
// the default stage-1 grid of a reduction and of a count: 2 blocks per CU
// (measured: reduce.hip); BK_REDUCE_BLOCKS overrides it for bk_reduce alone
constexpr int kRedBlocks = 512;
// the axis workspaces of reduce.hip and axis.hip: chunks x columns f64 partials
// (which set the width limit of a column reduction), then one ticket per
// column block (<= 2048 at 262144 columns)
constexpr int64_t kAxisWsDoubles = BK_MAX_AXIS0_COLUMNS;
constexpr int64_t kAxisTickets = 4096;
// waves of a block of the 16-B column kernels (reduce.hip colsum_tile_v, axis.hip col_stat_v)
constexpr int kColWaves = 16;

// min(the blocks `lanes` lanes of work need, `cap`), at least one (n = 0
// still launches: the fold writes the op's identity)
inline unsigned grid_blocks(int64_t lanes, int64_t cap) {
  const int64_t need = (lanes + kRedBlock - 1) / kRedBlock;
  return (unsigned)(need < 1 ? 1 : need < cap ? need : cap);
}

// bk_reduce on a kBool mask: op 0 the count of non-zero bytes, 3 any, 4 all (mask.hip)
int reduce_bool(int op, const void* a, int64_t n, void* workspace, void* out, hipStream_t stream);

template <typename T>
__device__ __forceinline__ void publish(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool take_last_ticket(unsigned* ticket, unsigned count) {
  __shared__ bool last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's partial stores have landed
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = prev == count - 1;
  }
  __syncthreads();
  return last;
}
template <typename T>
__device__ __forceinline__ T load_agent(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void rearm(unsigned* ticket) {
  __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace bk
