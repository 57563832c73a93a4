// lsmck_tableset.hip -- the opened table set on the GPU (gfx950):
// lsmck_tableset_open, SsTable::load (src/tokio/sstable.rs:32-55) for many
// tables at once, and lsmck_tableset_get_batch, Db::get
// (src/tokio/db.rs:156-189) over the set.  What a fence is and why it is
// exact: lsmck_tableset.h.
//
//   open  the point read's index pass (lsmck_sstget.hip, steps 1-3) over the
//         set's own buffers, then ts_fences: a lane per table walks its head
//         and its tail and leaves the two fence keys and their validity;
//         with "bloom_bits" > 0 then the tables' filters (lsmck_bloom.h):
//         ts_bloom_count, a lane per (table, interval), counts the keys,
//         ts_bloom_size scans the tables' blocks, ts_bloom_fill walks again
//         and ORs every key's eight bits into the zeroed filter buffer;
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
//         interval's walk (measured: DESIGN.md section 9).  On a set with
//         filters ts_hash hashes every query once, and ts_probe<true> tests a
//         pair that passed the fences against its table's block -- one
//         aligned 32-byte load -- before it is queued.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsmck.h"
#include "lsmck_device.h"
#include "lsmck_bloom.h"
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

// open with "bloom_bits" > 0, behind ts_fences and the index pass's read-back
// (the items are counted and no table was refused): a lane per (table,
// interval), `lanes` = the items + the tables.  Pass 1 walks and counts into
// nkeys[t], and marks in over[t] a table one of whose walks passes the cap.
__global__ __launch_bounds__(256) void ts_bloom_count(GetArgs a, uint64_t lanes, uint32_t cap,
                                                      unsigned long long* __restrict__ nkeys,
                                                      uint32_t* __restrict__ over) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= lanes) return;
  const uint64_t t = blm::interval_table(a.itemfirst, a.ntab, g);
  uint64_t n;
  if (!blm::count(get::table_at(a, t), g - blm::interval_first(a.itemfirst, t), cap, &n)) over[t] = 1u;
  if (n) atomicAdd(nkeys + t, (unsigned long long)n);
}

// ... the sizes: one workgroup scans the tables' blocks, 256 tables a step.
// desc[t] = the table's first block, its blocks and whether it has a filter;
// info[5] = the tables with a filter, [6] their keys, [7] their blocks.
__global__ __launch_bounds__(256) void ts_bloom_size(uint64_t ntab, uint32_t bits,
                                                     const unsigned long long* __restrict__ nkeys,
                                                     const uint32_t* __restrict__ over, blm::Desc* __restrict__ desc,
                                                     unsigned long long* __restrict__ info) {
  __shared__ uint64_t part[256];
  __shared__ uint64_t carry;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) carry = 0;
  uint64_t tables = 0, keys = 0;
  for (uint64_t base = 0; base < ntab; base += 256u) {
    const uint64_t t = base + tid;
    const uint32_t nb = t < ntab && !over[t] ? blm::nblocks_of(nkeys[t], bits) : 0u;
    part[tid] = nb;
    __syncthreads();
    for (uint32_t d = 1; d < 256u; d <<= 1) {  // inclusive scan of the step's blocks
      const uint64_t v = tid >= d ? part[tid - d] : 0u;
      __syncthreads();
      part[tid] += v;
      __syncthreads();
    }
    if (t < ntab) {
      blm::Desc D;
      D.first = nb ? carry + part[tid] - nb : 0u, D.nblocks = nb, D.valid = nb ? 1u : 0u;
      desc[t] = D;
      if (nb) ++tables, keys += nkeys[t];
    }
    __syncthreads();
    if (tid == 255u) carry += part[255];
    __syncthreads();
  }
  if (tables) atomicAdd(info + 5, (unsigned long long)tables), atomicAdd(info + 6, (unsigned long long)keys);
  if (tid == 0) info[7] = carry;
}

// ... pass 2, the filter buffer zeroed: the same walks, every visited record's
// key and the interval's item key hashed and ORed into the table's blocks
__global__ __launch_bounds__(256) void ts_bloom_fill(GetArgs a, uint64_t lanes, uint32_t cap,
                                                     const blm::Desc* __restrict__ desc, uint32_t* __restrict__ filt) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= lanes) return;
  const uint64_t t = blm::interval_table(a.itemfirst, a.ntab, g);
  const blm::Desc D = desc[t];
  if (D.valid) blm::fill(get::table_at(a, t), g - blm::interval_first(a.itemfirst, t), cap, filt, D);
}

// get on a set with filters: every query's hash, once per call (a query the
// call refuses is not read: its hash is 0 and nothing is looked up)
__global__ __launch_bounds__(256) void ts_hash(GetArgs a, uint64_t* __restrict__ qh) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const lsmck_get_query q = a.q[i];
  qh[i] = get::query_ok(q, a.qkeys_bytes) ? blm::hash(q.klen ? a.qkeys + q.key_off : a.qkeys, q.klen) : 0u;
}

// ts_probe<true>'s filters: the tables' descriptors, the blocks and the queries' hashes
template <bool kBloom>
struct TsBloom {};
template <>
struct TsBloom<true> {
  const blm::Desc* desc;
  const uint32_t* filt;
  const uint64_t* qh;
};
// the filter of table t drops query i: one aligned 32-byte load of the block
__device__ __forceinline__ bool ts_bloomed(const TsBloom<true>& b, uint64_t t, uint64_t i) {
  const blm::Desc D = b.desc[t];
  if (!D.valid) return false;
  const uint64_t h = b.qh[i];
  const uint4* p = (const uint4*)blm::block_at(b.filt, D, h);
  const uint4 lo = p[0], hi = p[1];
  const uint32_t w[blm::kWords] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return !blm::holds(w, h);
}
__device__ __forceinline__ bool ts_bloomed(const TsBloom<false>&, uint64_t, uint64_t) { return false; }

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
// registers more than 8 waves leave.)  ts_probe<false> is the probe of a set
// without filters; in ts_probe<true> a pair that passes the fences meets its
// table's filter before it is queued (ts_bloomed): info[9] = the pairs the
// filters dropped, counted as the fenced ones are.
template <bool kBloom>
__global__ __launch_bounds__(kTsBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void ts_probe(
    GetArgs a, const ts::Fence* __restrict__ fence, uint32_t iters, TsBloom<kBloom> bloom) {
  __shared__ uint64_t queue[kTsQueue];
  __shared__ uint32_t qn;
  __shared__ unsigned long long dropped;
  __shared__ unsigned long long bloomed;
  if (a.info[1] != kTsNo || a.info[5] != kTsNo) return;  // (the call fails: nothing is looked up; uniform)
  const uint32_t tid = threadIdx.x;
  if (tid == 0) qn = 0, dropped = 0;
  if (kBloom && tid == 0) bloomed = 0;
  __syncthreads();
  const uint64_t total = a.n * a.ntab;
  uint32_t mine = 0;  // the pairs of this thread the fences dropped
  uint32_t mineb = 0;  // ... and the filters
  const uint64_t chunk = (uint64_t)kTsBlock * iters;  // pairs per workgroup and pass
  for (uint64_t base = blockIdx.x * chunk; base < total; base += gridDim.x * chunk) {
    for (uint32_t it = 0; it < iters; ++it) {
      const uint64_t w = base + it * kTsBlock + tid;
      if (w < total) {
        const uint64_t t = w / a.n, i = w - t * a.n;
        if (ts::fenced(fence[t], get::key_at(a, i))) ++mine;
        else if (kBloom && ts_bloomed(bloom, t, i)) ++mineb;
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
    if (kBloom && mineb) atomicAdd(&bloomed, (unsigned long long)mineb);
    __syncthreads();
    if (tid == 0 && dropped) atomicAdd(a.info + 8, dropped);
    if (kBloom && tid == 0 && bloomed) atomicAdd(a.info + 9, bloomed);
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
extern "C" int lsmk_ts_bloom_count(const lsmck::GetArgs* a, uint64_t lanes, uint32_t cap, unsigned long long* nkeys,
                                   uint32_t* over, hipStream_t st) {
  if (lanes) hipLaunchKernelGGL(ts_bloom_count, dim3((unsigned)((lanes + 255u) / 256u)), dim3(256), 0, st, *a, lanes, cap, nkeys, over);
  return ts_launch_err();
}
extern "C" int lsmk_ts_bloom_size(uint64_t ntab, uint32_t bits, const unsigned long long* nkeys, const uint32_t* over,
                                  lsmck::blm::Desc* desc, unsigned long long* info, hipStream_t st) {
  hipLaunchKernelGGL(ts_bloom_size, dim3(1), dim3(256), 0, st, ntab, bits, nkeys, over, desc, info);
  return ts_launch_err();
}
extern "C" int lsmk_ts_bloom_fill(const lsmck::GetArgs* a, uint64_t lanes, uint32_t cap, const lsmck::blm::Desc* desc,
                                  uint32_t* filt, hipStream_t st) {
  if (lanes) hipLaunchKernelGGL(ts_bloom_fill, dim3((unsigned)((lanes + 255u) / 256u)), dim3(256), 0, st, *a, lanes, cap, desc, filt);
  return ts_launch_err();
}
extern "C" int lsmk_ts_hash(const lsmck::GetArgs* a, uint64_t* qh, hipStream_t st) {
  if (a->n) hipLaunchKernelGGL(ts_hash, dim3((unsigned)((a->n + 255u) / 256u)), dim3(256), 0, st, *a, qh);
  return ts_launch_err();
}
// desc == nullptr: a set without filters (ts_probe<false>); else filt and qh (lsmk_ts_hash) with it
extern "C" int lsmk_ts_pairs(const lsmck::GetArgs* a, const lsmck::ts::Fence* fence, const lsmck::blm::Desc* desc,
                             const uint32_t* filt, const uint64_t* qh, hipStream_t st) {
  if (a->ntab) {
    // a thread takes several pairs of a chunk only where that still leaves the whole grid: few pairs want every wave
    const uint64_t total = a->n * a->ntab, per = total / ((uint64_t)kTsBlock * kTsGrid);
    const uint32_t iters = per < 1u ? 1u : per > kTsIter ? kTsIter : (uint32_t)per;
    const uint64_t chunks = (total + kTsBlock * iters - 1u) / (kTsBlock * iters);
    const dim3 grid((unsigned)(chunks < kTsGrid ? chunks : kTsGrid));
    if (desc) {
      TsBloom<true> b;
      b.desc = desc, b.filt = filt, b.qh = qh;
      hipLaunchKernelGGL(ts_probe<true>, grid, dim3(kTsBlock), 0, st, *a, fence, iters, b);
    } else {
      hipLaunchKernelGGL(ts_probe<false>, grid, dim3(kTsBlock), 0, st, *a, fence, iters, TsBloom<false>());
    }
  }
  return ts_launch_err();
}
