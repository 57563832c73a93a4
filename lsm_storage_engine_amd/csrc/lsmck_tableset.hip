// lsmck_tableset.hip -- the opened table set on the GPU (gfx950):
// lsmck_tableset_open, SsTable::load (src/tokio/sstable.rs:32-55) for many
// tables at once, and lsmck_tableset_get_batch, Db::get
// (src/tokio/db.rs:156-189) over the set.  What a fence is and why it is
// exact: lsmck_tableset.h.
//
//   open  the point read's index pass (lsmck_sstget.hip, steps 1-3) over the
//         set's own buffers, then ts_fences: a lane per table walks its head
//         and its tail and leaves the two fence keys and their validity;
//   get   lsmck_db_get_batch's kernels (lsmck_dbget.hip) with the table
//         arrays pointing into the set, and in place of get_probe
//         ts_probe: the same (query, table) pairs, table major, a workgroup
//         taking a chunk of consecutive pairs a pass (1 to kTsIter per
//         thread: as many as still leave kTsGrid workgroups) and the next
//         chunk by the grid's stride.  The fence test comes first (two
//         compares of order keys, key bytes only on a tie past 8); the fences
//         are plain loads of an array of 80 bytes per table -- a wave's pairs
//         share one table or two, so its loads fall into one or two cache
//         lines.  The pairs that
//         pass are queued in LDS and looked up 256 at a time, in full waves:
//         then the winner check, get::table_get and the vector atomicMin, as
//         in get_probe.  Without the queue the few pairs a wide order leaves
//         lie one or two to a wave, and nearly every wave still waits for an
//         interval's walk (measured: DESIGN.md section 9).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsmck.h"
#include "lsmck_device.h"
#include "lsmck_tableset.h"

namespace lsmck {

constexpr unsigned long long kTsNo = ~0ull;
constexpr uint32_t kTsBlock = 256u;
constexpr uint32_t kTsIter = 16u;             // pairs per thread of a chunk, at most
constexpr uint32_t kTsGrid = 1u << 14;        // workgroups at most; the chunks beyond them by the grid's stride
constexpr uint32_t kTsQueue = 2u * kTsBlock;  // under kTsBlock entries wait, at most kTsBlock join them

// open: a lane per table.  info[3] / info[4] = the tables with a low / a high fence.
__global__ __launch_bounds__(256) void ts_fences(GetArgs a, ts::Fence* __restrict__ fence, uint32_t cap) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // (a refused table, or item scratch that has to grow: the open fails or runs again, nothing is walked)
  if (t >= a.ntab || a.info[0] != kTsNo || a.itemfirst[a.ntab] > a.nslots) return;
  const ts::Fence F = ts::fences(get::table_at(a, t), cap);
  fence[t] = F;
  if (F.valid & ts::kLow) atomicAdd(a.info + 3, 1ull);
  if (F.valid & ts::kHigh) atomicAdd(a.info + 4, 1ull);
}

// pair w behind the fences: get_probe's body
__device__ __forceinline__ void ts_lookup(const GetArgs& a, uint64_t w) {
  const uint64_t t = w / a.n, i = w - t * a.n;
  if (a.base + t > __atomic_load_n(a.win + i, __ATOMIC_RELAXED)) return;  // (a lower source answered already)
  const get::Table T = get::table_at(a, t);
  uint64_t vpos;
  uint32_t vlen;
  bool walked;
  if (get::table_get(T, get::key_at(a, i), &vpos, &vlen, &walked)) atomicMin(a.win + i, (uint32_t)(a.base + t));
  if (a.count) {
    atomicAdd(a.info + 3, 1ull);
    if (walked) atomicAdd(a.info + 4, 1ull);
  }
}

// get: the (query, table) pairs, table major: pair w = t * n + i.  info[8] =
// the pairs the fences dropped, counted before the winner check: the count
// does not depend on how the reads of win race.  (8 waves per SIMD as
// get_probe has: without the attribute the kernel takes a few scalar
// registers more than 8 waves leave.)
__global__ __launch_bounds__(kTsBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void ts_probe(
    GetArgs a, const ts::Fence* __restrict__ fence, uint32_t iters) {
  __shared__ uint64_t queue[kTsQueue];
  __shared__ uint32_t qn;
  __shared__ unsigned long long dropped;
  if (a.info[1] != kTsNo || a.info[5] != kTsNo) return;  // (the call fails: nothing is looked up; uniform)
  const uint32_t tid = threadIdx.x;
  if (tid == 0) qn = 0, dropped = 0;
  __syncthreads();
  const uint64_t total = a.n * a.ntab;
  uint32_t mine = 0;  // the pairs of this thread the fences dropped
  const uint64_t chunk = (uint64_t)kTsBlock * iters;  // pairs per workgroup and pass
  for (uint64_t base = blockIdx.x * chunk; base < total; base += gridDim.x * chunk) {
    for (uint32_t it = 0; it < iters; ++it) {
      const uint64_t w = base + it * kTsBlock + tid;
      if (w < total) {
        const uint64_t t = w / a.n, i = w - t * a.n;
        if (ts::fenced(fence[t], get::key_at(a, i))) ++mine;
        else queue[atomicAdd(&qn, 1u)] = w;  // (qn was under kTsBlock: the slot is under kTsQueue)
      }
      __syncthreads();
      const uint32_t have = qn;  // (no thread writes qn between the barriers around this read: `have` is uniform)
      __syncthreads();
      if (have >= kTsBlock) {  // a full block of lookups: the queue's top
        ts_lookup(a, queue[have - kTsBlock + tid]);
        if (tid == 0) qn = have - kTsBlock;
        __syncthreads();
      }
    }
    if (tid < qn) ts_lookup(a, queue[tid]);  // the chunk's rest
    __syncthreads();
    if (tid == 0) qn = 0;
    __syncthreads();
  }
  if (a.count) {  // one add per workgroup
    if (mine) atomicAdd(&dropped, (unsigned long long)mine);
    __syncthreads();
    if (tid == 0 && dropped) atomicAdd(a.info + 8, dropped);
  }
}

}  // namespace lsmck

using namespace lsmck;

static int ts_launch_err() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

extern "C" int lsmk_ts_fences(const lsmck::GetArgs* a, lsmck::ts::Fence* fence, uint32_t cap, hipStream_t st) {
  hipLaunchKernelGGL(ts_fences, dim3((unsigned)((a->ntab + 255u) / 256u)), dim3(256), 0, st, *a, fence, cap);
  return ts_launch_err();
}
extern "C" int lsmk_ts_pairs(const lsmck::GetArgs* a, const lsmck::ts::Fence* fence, hipStream_t st) {
  if (a->ntab) {
    // a thread takes several pairs of a chunk only where that still leaves the whole grid: few pairs want every wave
    const uint64_t total = a->n * a->ntab, per = total / ((uint64_t)kTsBlock * kTsGrid);
    const uint32_t iters = per < 1u ? 1u : per > kTsIter ? kTsIter : (uint32_t)per;
    const uint64_t chunks = (total + kTsBlock * iters - 1u) / (kTsBlock * iters);
    hipLaunchKernelGGL(ts_probe, dim3((unsigned)(chunks < kTsGrid ? chunks : kTsGrid)), dim3(kTsBlock), 0, st, *a, fence,
                       iters);
  }
  return ts_launch_err();
}
