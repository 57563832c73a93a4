// lsmck_memtable.hip -- batch memtable build on the GPU (gfx950):
// lsmck_memtable_build, the batch form of MemTable::from_log's map
// (src/memtable.rs:28-47), and lsmck_wal_recs_to_cmds, the adapter from the
// replay's compact records.  The step between the replay's records and
// lsmck_sstable_encode_batch's sorted entries: commands in log order -> the
// live entries in key order.
//   1. mem_validate: a thread per command; the first invalid one through the
//      64-bit atomicMin word.  Read back before anything else runs: no later
//      kernel reads a range it refused.
//   2. round r = 0, 1, ... over the positions still active (lsmck_memsort.h):
//      mem_chunk forms (chunk, tail) of the active elements, compacted in
//      order; rocPRIM's stable radix sort orders them by tail, then chunk,
//      then group (an index sort: the passes permute u32 slots, the next
//      pass's keys are gathered through them); mem_bound + a max-scan find the
//      runs' heads, mem_regroup writes the elements back to their positions
//      with the new groups and flags what stays active, a sum-scan and
//      mem_compact give the next round's positions and their count (8 bytes
//      to the host a round).
//   3. mem_resolve: the last element of each run of equal keys is the key's
//      last writer, live when it is an Insert; the mem_bytes shares reduced
//      per block, one 64-bit atomic add a block; a scan of the live flags
//      gives the slots; mem_emit writes ents and src after the host has seen
//      the count.
// Only the kernels here read key bytes or decide the result; rocPRIM sorts and
// scans fixed-width words.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <stdint.h>

#include <algorithm>

#include "lsmck.h"
#include "lsmck_device.h"
#include "lsmck_memsort.h"

namespace lsmck {

__global__ __launch_bounds__(256) void mem_validate(const lsmck_wal_cmd* __restrict__ cmds, uint64_t n, uint64_t kb,
                                                     uint64_t vb, unsigned long long* __restrict__ info) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!mem::valid(cmds[i], kb, vb)) atomicMin(info, (unsigned long long)i);
}

// before round 0: the log's order, every position active, one group
__global__ __launch_bounds__(256) void mem_init(MemWs W, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  W.perm[i] = (uint32_t)i;
  W.apos[i] = (uint32_t)i;
  W.grp[i] = 0;
  W.head[i] = 1;
}

// slot j < m: the element at the j-th active position
__global__ __launch_bounds__(256) void mem_chunk(MemWs W, const uint8_t* __restrict__ keys,
                                                  const lsmck_wal_cmd* __restrict__ cmds, uint64_t m, uint64_t r) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const uint32_t p = W.apos[j], c = W.perm[p];
  const uint64_t key_off = cmds[c].key_off;
  const uint32_t klen = cmds[c].klen;
  const mem::ChunkTail ct = mem::chunk_tail(keys, key_off, klen, r);
  W.chunk[j] = ct.chunk;
  W.tail[j] = (uint8_t)ct.tail;
  W.g[j] = W.grp[p];
  W.idx[j] = c;
}

// o: the sorted order of the slots.  bnd[i] = i where a run starts, else 0
__global__ __launch_bounds__(256) void mem_bound(MemWs W, const uint32_t* __restrict__ o, uint64_t m) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint32_t b = 0;
  if (i) {
    const uint32_t e = o[i], f = o[i - 1];
    if (!mem::same_run(W.g[e], W.chunk[e], W.tail[e], W.g[f], W.chunk[f], W.tail[f])) b = (uint32_t)i;
  }
  W.bnd[i] = b;
}

// hd[i] = the sorted slot where i's run starts.  The element goes back to the
// i-th active position with its run's head as its group; head[] = it starts a
// run; act[i] = it is refined further.
__global__ __launch_bounds__(256) void mem_regroup(MemWs W, const uint32_t* __restrict__ o, uint64_t m) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t e = o[i], h = W.hd[i];
  const bool first = h == i, last = i + 1 == m || W.hd[i + 1] == i + 1;
  const uint32_t p = W.apos[i];
  W.perm[p] = W.idx[e];
  W.head[p] = first ? 1 : 0;
  W.grp[p] = W.apos[h];
  W.act[i] = mem::stays_active(W.tail[e], !(first && last)) ? 1u : 0u;
}

// ex: the exclusive scan of act.  The next round's positions, in order, and their count
__global__ __launch_bounds__(256) void mem_compact(MemWs W, uint64_t m, unsigned long long* __restrict__ count) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t a = W.act[i], x = W.ex[i];
  if (a) W.apos2[x] = W.apos[i];
  if (i + 1 == m) *count = (unsigned long long)x + a;
}

// act[p] = position p is a live entry (act[n] = 0: the scan's total lands in
// ex[n]); *bytes += the block's mem_bytes shares
__global__ __launch_bounds__(256) void mem_resolve(MemWs W, const lsmck_wal_cmd* __restrict__ cmds, uint64_t n,
                                                    unsigned long long* __restrict__ bytes) {
  __shared__ uint64_t s[4];
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t x = 0;  // (two's complement: a Remove's share is negative, the whole sum never)
  if (p < n) {
    W.act[p] = mem::live(cmds, W.perm, W.head, n, p) ? 1u : 0u;
    x = (uint64_t)mem::contribution(cmds, W.perm, W.head, p);
  } else if (p == n) {
    W.act[p] = 0;
  }
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  if ((threadIdx.x & 63u) == 0) s[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint64_t t = s[0] + s[1] + s[2] + s[3];
    if (t) atomicAdd(bytes, (unsigned long long)t);
  }
}

__global__ __launch_bounds__(256) void mem_emit(MemWs W, const lsmck_wal_cmd* __restrict__ cmds, uint64_t n,
                                                 lsmck_wal_cmd* __restrict__ ents, uint32_t* __restrict__ src) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || !W.act[p]) return;
  const uint32_t j = W.ex[p], c = W.perm[p];
  lsmck_wal_cmd e = cmds[c];
  e.type = 1u;
  e.reserved = 0u;
  ents[j] = e;
  if (src) src[j] = c;
}

__global__ __launch_bounds__(256) void mem_recs_to_cmds(const lsmck_wal_rec16* __restrict__ recs, uint64_t n,
                                                         uint64_t img_bytes, lsmck_wal_cmd* __restrict__ cmds) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  cmds[i] = mem::rec_to_cmd(recs[i], img_bytes);
}

// the next sort pass's keys, gathered through the order so far
struct MemGather64 {
  const uint64_t* v;
  __host__ __device__ uint64_t operator()(uint32_t j) const { return v[j]; }
};
struct MemGather32 {
  const uint32_t* v;
  __host__ __device__ uint32_t operator()(uint32_t j) const { return v[j]; }
};

}  // namespace lsmck

using namespace lsmck;

static int mem_err(hipError_t e) { return e == hipSuccess ? 0 : -(int)e; }
static int mem_launch_err() { return mem_err(hipGetLastError()); }
static unsigned mem_grid(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

// the workspace's arrays for n commands (ws == nullptr: the size alone)
extern "C" size_t lsmk_mem_carve(uint8_t* ws, uint64_t n, MemWs* W) {
  size_t at = 0;
  auto take = [&](size_t bytes) {
    uint8_t* p = ws ? ws + at : nullptr;
    at += (bytes + 255u) & ~(size_t)255u;
    return p;
  };
  MemWs w;
  w.chunk = (uint64_t*)take(8 * n);
  w.kout = (uint64_t*)take(8 * n);
  w.perm = (uint32_t*)take(4 * n);
  w.grp = (uint32_t*)take(4 * n);
  w.apos = (uint32_t*)take(4 * n);
  w.apos2 = (uint32_t*)take(4 * n);
  w.g = (uint32_t*)take(4 * n);
  w.idx = (uint32_t*)take(4 * n);
  w.o1 = (uint32_t*)take(4 * n);
  w.o2 = (uint32_t*)take(4 * n);
  w.o3 = (uint32_t*)take(4 * n);
  w.bnd = (uint32_t*)take(4 * n);
  w.hd = (uint32_t*)take(4 * n);
  w.act = (uint32_t*)take(4 * (n + 1));
  w.ex = (uint32_t*)take(4 * (n + 1));
  w.tail = (uint8_t*)take(n);
  w.head = (uint8_t*)take(n);
  if (W) *W = w;
  return at;
}

extern "C" int lsmk_mem_validate(const lsmck_wal_cmd* cmds, uint64_t n, uint64_t keys_bytes, uint64_t vals_bytes,
                                 unsigned long long* info, hipStream_t st) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(mem_validate, dim3(mem_grid(n)), dim3(256), 0, st, cmds, n, keys_bytes, vals_bytes, info);
  return mem_launch_err();
}

extern "C" int lsmk_mem_init(const MemWs* W, uint64_t n, hipStream_t st) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(mem_init, dim3(mem_grid(n)), dim3(256), 0, st, *W, n);
  return mem_launch_err();
}

extern "C" int lsmk_mem_chunk(const MemWs* W, const uint8_t* keys, const lsmck_wal_cmd* cmds, uint64_t m, uint64_t r,
                              hipStream_t st) {
  hipLaunchKernelGGL(mem_chunk, dim3(mem_grid(m)), dim3(256), 0, st, *W, keys, cmds, m, r);
  return mem_launch_err();
}

// The round's fixed-width part over the m slots mem_chunk filled: the stable
// sort by (group, chunk, tail) -- round 0 has one group --, the runs, the
// elements back in place, the next round's positions in W->apos2 and their
// count in *count.  tmp == nullptr: *tmp_bytes = the temporary storage the
// round needs (rocPRIM's two-call protocol, the largest of its calls).
extern "C" int lsmk_mem_sort_regroup(const MemWs* Wp, uint64_t m, uint64_t r, unsigned group_bits, void* tmp,
                                     size_t* tmp_bytes, unsigned long long* count, hipStream_t st) {
  const MemWs& W = *Wp;
  const bool query = tmp == nullptr;
  size_t need = 0, b;
  rocprim::counting_iterator<uint32_t> iota(0u);
  auto k2 = rocprim::make_transform_iterator(W.o1, MemGather64{W.chunk});
  auto k3 = rocprim::make_transform_iterator(W.o2, MemGather32{W.g});
  const uint32_t* o = r ? W.o3 : W.o2;
  hipError_t e;
  b = query ? 0 : *tmp_bytes;
  if ((e = rocprim::radix_sort_pairs(tmp, b, W.tail, (uint8_t*)W.kout, iota, W.o1, m, 0, 4, st)) != hipSuccess)
    return mem_err(e);
  need = std::max(need, b);
  b = query ? 0 : *tmp_bytes;
  if ((e = rocprim::radix_sort_pairs(tmp, b, k2, W.kout, W.o1, W.o2, m, 0, 64, st)) != hipSuccess) return mem_err(e);
  need = std::max(need, b);
  if (r) {
    b = query ? 0 : *tmp_bytes;
    if ((e = rocprim::radix_sort_pairs(tmp, b, k3, (uint32_t*)W.kout, W.o2, W.o3, m, 0, group_bits, st)) !=
        hipSuccess)
      return mem_err(e);
    need = std::max(need, b);
  }
  if (!query) {
    hipLaunchKernelGGL(mem_bound, dim3(mem_grid(m)), dim3(256), 0, st, W, o, m);
    if (int rc = mem_launch_err()) return rc;
  }
  b = query ? 0 : *tmp_bytes;
  if ((e = rocprim::inclusive_scan(tmp, b, W.bnd, W.hd, m, rocprim::maximum<uint32_t>(), st)) != hipSuccess)
    return mem_err(e);
  need = std::max(need, b);
  if (!query) {
    hipLaunchKernelGGL(mem_regroup, dim3(mem_grid(m)), dim3(256), 0, st, W, o, m);
    if (int rc = mem_launch_err()) return rc;
  }
  b = query ? 0 : *tmp_bytes;
  if ((e = rocprim::exclusive_scan(tmp, b, W.act, W.ex, 0u, m, rocprim::plus<uint32_t>(), st)) != hipSuccess)
    return mem_err(e);
  need = std::max(need, b);
  if (query) {
    *tmp_bytes = std::max<size_t>(need, 1);
    return 0;
  }
  hipLaunchKernelGGL(mem_compact, dim3(mem_grid(m)), dim3(256), 0, st, W, m, count);
  return mem_launch_err();
}

// the live flags, *bytes += mem_bytes, the slots; ex[n] = the live entries.
// tmp == nullptr: *tmp_bytes alone
extern "C" int lsmk_mem_resolve(const MemWs* Wp, const lsmck_wal_cmd* cmds, uint64_t n, void* tmp, size_t* tmp_bytes,
                                unsigned long long* bytes, hipStream_t st) {
  const MemWs& W = *Wp;
  const bool query = tmp == nullptr;
  if (!query) {
    hipLaunchKernelGGL(mem_resolve, dim3(mem_grid(n + 1)), dim3(256), 0, st, W, cmds, n, bytes);
    if (int rc = mem_launch_err()) return rc;
  }
  size_t b = query ? 0 : *tmp_bytes;
  hipError_t e = rocprim::exclusive_scan(tmp, b, W.act, W.ex, 0u, n + 1, rocprim::plus<uint32_t>(), st);
  if (e != hipSuccess) return mem_err(e);
  if (query) *tmp_bytes = std::max<size_t>(b, 1);
  return 0;
}

extern "C" int lsmk_mem_emit(const MemWs* W, const lsmck_wal_cmd* cmds, uint64_t n, lsmck_wal_cmd* ents, uint32_t* src,
                             hipStream_t st) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(mem_emit, dim3(mem_grid(n)), dim3(256), 0, st, *W, cmds, n, ents, src);
  return mem_launch_err();
}

extern "C" int lsmk_mem_recs_to_cmds(const lsmck_wal_rec16* recs, uint64_t n, uint64_t img_bytes, lsmck_wal_cmd* cmds,
                                     hipStream_t st) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(mem_recs_to_cmds, dim3(mem_grid(n)), dim3(256), 0, st, recs, n, img_bytes, cmds);
  return mem_launch_err();
}
