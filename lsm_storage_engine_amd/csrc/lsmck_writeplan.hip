// lsmck_writeplan.hip -- the batch write plan on the GPU (gfx950):
// lsmck_db_write_plan, the batch form of LsmStorage::insert / delete's memtable
// side (src/sync/lsm_storage.rs:59-78, 133-139).  A command stream is cut where
// the reference would flush, and every cut becomes the flushed memtable's
// entries in key order; the rule is lsmck_writeplan.h's.
//   1. order: the memtable build's rounds (lsmck_memtable.hip, unchanged) leave
//      the commands by (key, log position); wpl_prep turns that into prev -- the
//      command before with the same key -- and a packed (a, is Insert) word per
//      command, so that a walk step reads two coalesced words.
//   2. wpl_walk: a thread per candidate start walks its memtable for at most
//      cut_walk_cap commands: a cut, the end of the log, or LONG.
//   3. wpl_exit: the starts in blocks of cut_block; per block, in LDS, pointer
//      doubling over the in-block successors: where every start's orbit leaves
//      the block or meets a start that is not a cut.  wpl_chain: one workgroup
//      follows the orbit of command 0 from exit to exit, notes where it enters a
//      block, and resolves a LONG start by windows of its width -- a block scan
//      carries bytes, a min-reduction finds the first qualifying Insert.
//      wpl_mark: per block, a thread per entry point chases the in-block
//      successors through LDS and marks the true starts.
//   4. emit: an inclusive scan of the marks numbers the segments; wpl_flag
//      finds the last position of every (segment, key), a scan gives the count;
//      after the host has seen the counts wpl_compact, a stable radix sort by
//      segment and wpl_emit / wpl_segs write ents, src and segs.
// Only the kernels here decide the result; rocPRIM sorts and scans fixed-width
// words.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>

#include <algorithm>

#include "lsmck.h"
#include "lsmck_device.h"
#include "lsmck_writeplan.h"

namespace lsmck {

constexpr unsigned kWplWide = 1024;  // wpl_exit's and wpl_chain's workgroup: 8 links a thread at cut_block 8192
constexpr unsigned kWplPer = 8;

// info[0]: the first command whose entry would be too long (atomic min);
// info[1]: a delete is there and the tombstone byte (tomb; null: past the
// arena) is missing or not 0
__global__ __launch_bounds__(256) void wpl_check(const lsmck_wal_cmd* __restrict__ cmds, uint64_t n,
                                                  const uint8_t* __restrict__ tomb,
                                                  unsigned long long* __restrict__ info) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const lsmck_wal_cmd c = cmds[i];
  if (!wpl::fits(c)) atomicMin(info, (unsigned long long)i);
  if (c.type == 2u && wpl::tomb_bad(tomb, tomb ? 1u : 0u, 0)) atomicMax(info + 1, 1ull);
}

__global__ __launch_bounds__(256) void wpl_prep(WplWs P, const lsmck_wal_cmd* __restrict__ cmds, uint64_t n) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  P.prev[P.perm[p]] = wpl::prev_of(P.perm, P.head, p);
  P.aw[p] = wpl::pack(cmds[p]);
  P.mark[p] = 0;
}

__global__ __launch_bounds__(256) void wpl_walk(WplWs P, uint64_t n, uint64_t limit, uint32_t cap,
                                                 unsigned long long* __restrict__ steps) {
  __shared__ uint64_t part[4];
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t x = 0;
  if (s < n) {
    const wpl::Walk w = wpl::walk(P.aw, P.prev, n, s, limit, cap);
    P.nxt[s] = w.nxt;
    P.byt[s] = w.bytes;
    P.state[s] = w.state;
    x = w.steps;
  }
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(steps, (unsigned long long)(part[0] + part[1] + part[2] + part[3]));
}

// block b's starts [b0, b1): lnk[i] = the in-block successor of start b0 + i,
// or i itself where the orbit leaves the block or the start is not a cut
__device__ __forceinline__ uint32_t wpl_link(const WplWs& P, uint64_t b0, uint64_t b1, uint32_t i) {
  const uint64_t s = b0 + i;
  const uint32_t nx = P.nxt[s];
  return wpl::follows(P.state[s], nx, b1) ? (uint32_t)(nx - b0) : i;
}

// exitp[s] = the last start of s's orbit inside s's block
__global__ __launch_bounds__(kWplWide) void wpl_exit(WplWs P, uint64_t n, uint32_t B) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lnk[];
  const uint64_t b0 = (uint64_t)blockIdx.x * B;
  const uint32_t cnt = (uint32_t)((n - b0 < B) ? n - b0 : B);
  for (uint32_t i = threadIdx.x; i < cnt; i += kWplWide) lnk[i] = wpl_link(P, b0, b0 + cnt, i);
  __syncthreads();
  for (;;) {  // at most log2(cnt) + 1 rounds: every round doubles the hops a link spans
    uint32_t t[kWplPer];
    int changed = 0;
#pragma unroll
    for (unsigned k = 0; k < kWplPer; ++k) {
      const uint32_t i = threadIdx.x + k * kWplWide;
      t[k] = 0;
      if (i < cnt) {
        const uint32_t a = lnk[i];
        t[k] = lnk[a];
        changed |= t[k] != a;
      }
    }
    changed = __syncthreads_or(changed);
#pragma unroll
    for (unsigned k = 0; k < kWplPer; ++k) {
      const uint32_t i = threadIdx.x + k * kWplWide;
      if (i < cnt) lnk[i] = t[k];
    }
    __syncthreads();
    if (!changed) break;
  }
  for (uint32_t i = threadIdx.x; i < cnt; i += kWplWide) P.exitp[b0 + i] = (uint32_t)(b0 + lnk[i]);
}

// One workgroup: the true starts' orbit from command 0, from block exit to
// block exit.  elist[0 .. cinfo[0]): where it enters a block or goes on behind
// a LONG start, increasing; bfirst[b]: the first of them in block b.  cinfo:
// [0] the entry points, [1] the LONG starts resolved, [2] the last command
// closed its memtable, [3] elist was too small (nothing past ecap is written).
__global__ __launch_bounds__(kWplWide) void wpl_chain(WplWs P, uint64_t n, uint32_t B, uint64_t limit,
                                                       uint32_t* __restrict__ elist, uint32_t ecap,
                                                       uint32_t* __restrict__ bfirst,
                                                       unsigned long long* __restrict__ cinfo) {
  __shared__ uint64_t wsum[kWplWide / 64];
  __shared__ unsigned long long first;
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint64_t s = 0, in_block = ~0ull;  // the block the last entry point lies in
  uint32_t ne = 0, nl = 0;
  bool closed = true, over = false;
  while (s < n) {
    if (ne >= ecap) {
      over = true;
      break;
    }
    const uint64_t b = s / B;
    if (tid == 0) {
      elist[ne] = (uint32_t)s;
      if (b != in_block) bfirst[b] = ne;
    }
    in_block = b;
    ++ne;
    const uint32_t e = P.exitp[s];
    const uint8_t st = P.state[e];
    if (st == wpl::kCut) {
      s = P.nxt[e];
      continue;
    }
    if (st == wpl::kOpen) {
      closed = false;
      break;
    }
    // a LONG start: its memtable by windows of the workgroup's width
    ++nl;
    uint64_t carry = 0, found = ~0ull;
    for (uint64_t base = e; base < n; base += kWplWide) {
      const uint64_t j = base + tid;
      uint64_t w = 0, x = 0;
      if (j < n) {
        w = P.aw[j];
        x = wpl::delta(P.aw, P.prev, e, j);
      }
      for (int d = 1; d < 64; d <<= 1) {  // the wave's inclusive scan
        const uint64_t y = __shfl_up(x, d, 64);
        if ((int)lane >= d) x += y;
      }
      if (lane == 63u) wsum[wave] = x;
      if (tid == 0) first = ~0ull;
      __syncthreads();
      uint64_t before = 0, total = 0;
      for (unsigned k = 0; k < kWplWide / 64; ++k) {
        const uint64_t v = wsum[k];
        if (k < wave) before += v;
        total += v;
      }
      const uint64_t bytes = carry + before + x;
      unsigned long long cand = (j < n && wpl::qualifies(w, bytes, limit)) ? (unsigned long long)j : ~0ull;
      for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(cand, d, 64);
        cand = o < cand ? o : cand;
      }
      if (lane == 0 && cand != ~0ull) atomicMin(&first, cand);
      __syncthreads();
      const unsigned long long m = first;
      if (m != ~0ull) {
        if (j == m) {
          P.byt[e] = bytes;
          P.nxt[e] = (uint32_t)(m + 1u);
          P.state[e] = wpl::kLongCut;
        }
        found = m;
      }
      carry += total;
      __syncthreads();  // (wsum and first are written again by the next window)
      if (found != ~0ull) break;
    }
    if (found == ~0ull) {
      if (tid == 0) {
        P.byt[e] = carry;
        P.nxt[e] = (uint32_t)n;
        P.state[e] = wpl::kLongOpen;
      }
      closed = false;
      break;
    }
    s = found + 1u;
  }
  if (tid == 0) {
    cinfo[0] = ne;
    cinfo[1] = nl;
    cinfo[2] = closed ? 1u : 0u;
    cinfo[3] = over ? 1u : 0u;
  }
}

// per block: from each of its entry points along the in-block successors
__global__ __launch_bounds__(256) void wpl_mark(WplWs P, uint64_t n, uint32_t B, const uint32_t* __restrict__ elist,
                                                 const unsigned long long* __restrict__ cinfo,
                                                 const uint32_t* __restrict__ bfirst) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lnk[];
  const uint32_t f = bfirst[blockIdx.x];
  if (f == wpl::kNone) return;  // (no true start lies in this block)
  const uint64_t b0 = (uint64_t)blockIdx.x * B;
  const uint32_t cnt = (uint32_t)((n - b0 < B) ? n - b0 : B);
  for (uint32_t i = threadIdx.x; i < cnt; i += blockDim.x) lnk[i] = wpl_link(P, b0, b0 + cnt, i);
  __syncthreads();
  const uint64_t ne = cinfo[0];
  for (uint64_t k = (uint64_t)f + threadIdx.x; k < ne; k += blockDim.x) {
    const uint64_t s = elist[k];
    if (s >= b0 + cnt) break;
    uint32_t i = (uint32_t)(s - b0);
    for (;;) {
      P.mark[b0 + i] = 1u;
      const uint32_t nx = lnk[i];
      if (nx == i) break;
      i = nx;
    }
  }
}

// act[p] = position p of the order is an entry (act[n] = 0: the scan's total lands in ex[n])
__global__ __launch_bounds__(256) void wpl_flag(WplWs P, uint64_t n) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n)
    P.act[p] = wpl::is_entry(P.perm, P.head, P.seg1, n, p) ? 1u : 0u;
  else if (p == n)
    P.act[p] = 0;
}

// the entries in key order: their segment (the sort's key) and their command
__global__ __launch_bounds__(256) void wpl_compact(WplWs P, uint64_t n) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || !P.act[p]) return;
  const uint32_t j = P.ex[p], c = P.perm[p];
  P.ekey[j] = P.seg1[c] - 1u;
  P.eval[j] = c;
}

// skey / sval: the entries by (segment, key)
__global__ __launch_bounds__(256) void wpl_emit(WplWs P, const lsmck_wal_cmd* __restrict__ cmds, uint64_t nent,
                                                 uint64_t tomb_off, lsmck_wal_cmd* __restrict__ ents,
                                                 uint32_t* __restrict__ src, lsmck_write_seg* __restrict__ segs) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nent) return;
  const uint32_t c = P.sval[j], g = P.skey[j];
  ents[j] = wpl::entry(cmds[c], tomb_off);
  if (src) src[j] = c;
  if (j == 0 || P.skey[j - 1] != g) segs[g].first_ent = j;
}

// a true start's segment: its first command and size_in_bytes() at its end;
// thread n: the empty open segment behind a last command that flushed
__global__ __launch_bounds__(256) void wpl_segs(WplWs P, uint64_t n, uint64_t nent, uint64_t nseg, int closed,
                                                 lsmck_write_seg* __restrict__ segs) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n) {
    if (!P.mark[c]) return;
    const uint32_t g = P.seg1[c] - 1u;
    segs[g].first_cmd = c;
    segs[g].mem_bytes = P.byt[c];
  } else if (c == n && closed) {
    lsmck_write_seg z;
    z.first_cmd = n;
    z.first_ent = nent;
    z.mem_bytes = 0;
    segs[nseg] = z;
  }
}

}  // namespace lsmck

using namespace lsmck;

static int wpl_err(hipError_t e) { return e == hipSuccess ? 0 : -(int)e; }
static int wpl_launch_err() { return wpl_err(hipGetLastError()); }
static unsigned wpl_grid(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

// the plan's arrays, laid over the memtable build's workspace once its rounds
// are done: perm and head stay, every other array is free
extern "C" void lsmk_wpl_carve(const MemWs* W, WplWs* P) {
  P->perm = W->perm;
  P->head = W->head;
  P->aw = W->chunk;
  P->byt = W->kout;
  P->prev = W->grp;
  P->nxt = W->apos;
  P->exitp = W->g;
  P->mark = W->bnd;
  P->seg1 = W->hd;
  P->act = W->act;
  P->ex = W->ex;
  P->ekey = W->idx;
  P->eval = W->o1;
  P->skey = W->o2;
  P->sval = W->o3;
  P->state = W->tail;
}

extern "C" int lsmk_wpl_check(const lsmck_wal_cmd* cmds, uint64_t n, const uint8_t* tomb, unsigned long long* info,
                              hipStream_t st) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(wpl_check, dim3(wpl_grid(n)), dim3(256), 0, st, cmds, n, tomb, info);
  return wpl_launch_err();
}

extern "C" int lsmk_wpl_prep(const WplWs* P, const lsmck_wal_cmd* cmds, uint64_t n, hipStream_t st) {
  hipLaunchKernelGGL(wpl_prep, dim3(wpl_grid(n)), dim3(256), 0, st, *P, cmds, n);
  return wpl_launch_err();
}

extern "C" int lsmk_wpl_walk(const WplWs* P, uint64_t n, uint64_t limit, uint32_t cap, unsigned long long* steps,
                             hipStream_t st) {
  hipLaunchKernelGGL(wpl_walk, dim3(wpl_grid(n)), dim3(256), 0, st, *P, n, limit, cap, steps);
  return wpl_launch_err();
}

// block: 64..8192 starts.  elist: ecap words; bfirst: a word per block, set to
// 0xFF bytes here; cinfo: four words
extern "C" int lsmk_wpl_chain(const WplWs* P, uint64_t n, uint32_t block, uint64_t limit, uint32_t* elist,
                              uint32_t ecap, uint32_t* bfirst, unsigned long long* cinfo, hipStream_t st) {
  if (block < 64u || block > kWplWide * kWplPer) return wpl_err(hipErrorInvalidValue);
  const unsigned nblk = (unsigned)((n + block - 1u) / block);
  hipError_t e = hipMemsetAsync(bfirst, 0xFF, 4 * (size_t)nblk, st);
  if (e != hipSuccess) return wpl_err(e);
  hipLaunchKernelGGL(wpl_exit, dim3(nblk), dim3(kWplWide), 4 * (size_t)block, st, *P, n, block);
  if (int rc = wpl_launch_err()) return rc;
  hipLaunchKernelGGL(wpl_chain, dim3(1), dim3(kWplWide), 0, st, *P, n, block, limit, elist, ecap, bfirst, cinfo);
  return wpl_launch_err();
}

// the marks, the segment numbers, the entry flags and their slots: ex[n] = the
// entries, seg1[n - 1] = the segments that hold a command.  tmp == nullptr:
// *tmp_bytes alone
extern "C" int lsmk_wpl_mark(const WplWs* Pp, uint64_t n, uint32_t block, const uint32_t* elist,
                             const unsigned long long* cinfo, const uint32_t* bfirst, void* tmp, size_t* tmp_bytes,
                             hipStream_t st) {
  const WplWs& P = *Pp;
  const bool query = tmp == nullptr;
  size_t need = 0, b;
  hipError_t e;
  if (!query) {
    const unsigned nblk = (unsigned)((n + block - 1u) / block);
    hipLaunchKernelGGL(wpl_mark, dim3(nblk), dim3(256), 4 * (size_t)block, st, P, n, block, elist, cinfo, bfirst);
    if (int rc = wpl_launch_err()) return rc;
  }
  b = query ? 0 : *tmp_bytes;
  if ((e = rocprim::inclusive_scan(tmp, b, P.mark, P.seg1, n, rocprim::plus<uint32_t>(), st)) != hipSuccess)
    return wpl_err(e);
  need = std::max(need, b);
  if (!query) {
    hipLaunchKernelGGL(wpl_flag, dim3(wpl_grid(n + 1)), dim3(256), 0, st, P, n);
    if (int rc = wpl_launch_err()) return rc;
  }
  b = query ? 0 : *tmp_bytes;
  if ((e = rocprim::exclusive_scan(tmp, b, P.act, P.ex, 0u, n + 1, rocprim::plus<uint32_t>(), st)) != hipSuccess)
    return wpl_err(e);
  need = std::max(need, b);
  if (query) *tmp_bytes = std::max<size_t>(need, 1);
  return 0;
}

// lsmk_wpl_mark's first half alone, for lsmck_db_apply_plan, whose entry flags
// are its own: the marks and the segment numbers
extern "C" int lsmk_wpl_number(const WplWs* Pp, uint64_t n, uint32_t block, const uint32_t* elist,
                               const unsigned long long* cinfo, const uint32_t* bfirst, void* tmp, size_t* tmp_bytes,
                               hipStream_t st) {
  const WplWs& P = *Pp;
  const bool query = tmp == nullptr;
  if (!query) {
    const unsigned nblk = (unsigned)((n + block - 1u) / block);
    hipLaunchKernelGGL(wpl_mark, dim3(nblk), dim3(256), 4 * (size_t)block, st, P, n, block, elist, cinfo, bfirst);
    if (int rc = wpl_launch_err()) return rc;
  }
  size_t b = query ? 0 : *tmp_bytes;
  const hipError_t e = rocprim::inclusive_scan(tmp, b, P.mark, P.seg1, n, rocprim::plus<uint32_t>(), st);
  if (e != hipSuccess) return wpl_err(e);
  if (query) *tmp_bytes = std::max<size_t>(b, 1);
  return 0;
}

// ents, src (optional) and segs (nseg items, one more behind a last command
// that flushed: closed).  tmp == nullptr: *tmp_bytes alone
extern "C" int lsmk_wpl_emit(const WplWs* Pp, const lsmck_wal_cmd* cmds, uint64_t n, uint64_t nent, uint64_t nseg,
                             int closed, uint64_t tomb_off, lsmck_wal_cmd* ents, uint32_t* src, lsmck_write_seg* segs,
                             void* tmp, size_t* tmp_bytes, hipStream_t st) {
  const WplWs& P = *Pp;
  const bool query = tmp == nullptr;
  unsigned bits = 1;
  while (bits < 32 && ((uint64_t)1 << bits) < nseg) ++bits;
  if (!query) {
    hipLaunchKernelGGL(wpl_compact, dim3(wpl_grid(n)), dim3(256), 0, st, P, n);
    if (int rc = wpl_launch_err()) return rc;
  }
  size_t b = query ? 0 : *tmp_bytes;
  const hipError_t e = rocprim::radix_sort_pairs(tmp, b, P.ekey, P.skey, P.eval, P.sval, nent, 0, bits, st);
  if (e != hipSuccess) return wpl_err(e);
  if (query) {
    *tmp_bytes = std::max<size_t>(b, 1);
    return 0;
  }
  hipLaunchKernelGGL(wpl_emit, dim3(wpl_grid(nent)), dim3(256), 0, st, P, cmds, nent, tomb_off, ents, src, segs);
  if (int rc = wpl_launch_err()) return rc;
  hipLaunchKernelGGL(wpl_segs, dim3(wpl_grid(n + 1)), dim3(256), 0, st, P, n, nent, nseg, closed, segs);
  return wpl_launch_err();
}
