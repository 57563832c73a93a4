// lsmck_apply.hip -- the batch command stream on the GPU (gfx950):
// lsmck_db_apply_plan, the write plan (lsmck_writeplan.hip) with Gets between
// the writes, each answered by the last write in front of it
// (LsmStorage::get, src/sync/lsm_storage.rs:99-125); the rule is
// lsmck_apply.h's.  The memtable build's rounds, the walk, the chain, the
// marks and their scan, the compaction, the sort by segment and the emit are
// the write plan's kernels, unchanged.  The kernels here are the four pieces
// that look at a key's run in the order by (key, log position), where Gets now
// stand between the writes:
//   1. apl_validate: a command is a write the build takes or a Get whose key
//      lies in the arena; the entry-length and tombstone-byte rules hold for
//      writes.
//   2. prep: apl_pack writes the packed words by command (a Get's is 0) and
//      clears the marks; apl_events forms, per position of the order, the two
//      words whose inclusive max-scans give the run's start and the last
//      write; apl_prev turns them into prev (a write's previous write), ans
//      (the write that answers a Get) and pq (that write's position).
//   3. entry flags: every write starts as an entry (apl_prev); apl_clear lets a
//      write whose previous write has its segment clear that one's flag -- one
//      writer a flag, no atomics.
//   4. gets out: apl_slots flags the Gets and the misses in stream order, two
//      exclusive scans give their slots and, through apl_totals, both counts;
//      apl_gets writes gets, miss_q and miss_get.
// Only the kernels decide the result; rocPRIM scans fixed-width words.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>

#include <algorithm>

#include "lsmck.h"
#include "lsmck_apply.h"
#include "lsmck_device.h"

namespace lsmck {

__global__ __launch_bounds__(256) void apl_validate(const lsmck_wal_cmd* __restrict__ cmds, uint64_t n, uint64_t kb,
                                                     uint64_t vb, const uint8_t* __restrict__ tomb,
                                                     unsigned long long* __restrict__ info) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const lsmck_wal_cmd c = cmds[i];
  if (!apl::valid(c, kb, vb) || !apl::fits(c)) atomicMin(info, (unsigned long long)i);
  if (c.type == 2u && wpl::tomb_bad(tomb, tomb ? 1u : 0u, 0)) atomicMax(info + 1, 1ull);
}

__global__ __launch_bounds__(256) void apl_pack(WplWs P, const lsmck_wal_cmd* __restrict__ cmds, uint64_t n) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  P.aw[c] = apl::pack(cmds[c]);
  P.mark[c] = 0;
}

__global__ __launch_bounds__(256) void apl_events(WplWs P, AplWs A, uint64_t n) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  A.eh[p] = apl::head_word(P.head, p);
  A.ew[p] = apl::write_word(!apl::word_is_get(P.aw[P.perm[p]]), p);
}

// (pq lies over eh, which nothing reads any more; act[n] = 0: the scan's total lands in ex[n])
__global__ __launch_bounds__(256) void apl_prev(WplWs P, AplWs A, uint64_t n) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p > n) return;
  if (p == n) {
    P.act[p] = 0;
    return;
  }
  const uint32_t c = P.perm[p];
  const bool write = !apl::word_is_get(P.aw[c]);
  const uint32_t q = apl::prev_pos(A.rs, A.lw, p);
  const uint32_t pc = q == apl::kNone ? apl::kNone : P.perm[q];
  P.prev[c] = write ? pc : apl::kNone;
  A.ans[c] = pc;
  A.pq[p] = write ? q : apl::kNone;
  P.act[p] = write ? 1u : 0u;
}

__global__ __launch_bounds__(256) void apl_clear(WplWs P, AplWs A, uint64_t n) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint32_t q = A.pq[p];
  if (q != apl::kNone && apl::replaces(P.seg1, P.perm[p], P.perm[q])) P.act[q] = 0;
}

__global__ __launch_bounds__(256) void apl_slots(WplWs P, AplWs A, uint64_t n) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const bool get = apl::word_is_get(P.aw[c]);
  A.gf[c] = get ? 1u : 0u;
  A.mf[c] = (get && A.ans[c] == apl::kNone) ? 1u : 0u;
}

// the two totals behind the exclusive scans (no word of the stream is counted with atomics: a count a wave on one
// address costs more than both scans)
__global__ void apl_totals(AplWs A, uint64_t n, unsigned long long* __restrict__ info) {
  if (blockIdx.x || threadIdx.x) return;
  info[7] = (unsigned long long)A.gslot[n - 1] + A.gf[n - 1];
  info[8] = (unsigned long long)A.mslot[n - 1] + A.mf[n - 1];
}

__global__ __launch_bounds__(256) void apl_gets(WplWs P, AplWs A, const lsmck_wal_cmd* __restrict__ cmds,
                                                 const uint8_t* __restrict__ vals, uint64_t n, uint64_t tomb_off,
                                                 lsmck_apply_get* __restrict__ gets,
                                                 lsmck_get_query* __restrict__ miss_q, uint32_t* __restrict__ miss_get) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const lsmck_wal_cmd cmd = cmds[c];
  if (!apl::is_get(cmd)) return;
  const uint32_t j = A.ans[c], slot = A.gslot[c];
  gets[slot] = apl::answer(cmds, vals, tomb_off, (uint32_t)c, j,
                           j == apl::kNone ? LSMCK_GET_NONE : apl::source(P.seg1, (uint32_t)c, j));
  if (j == apl::kNone && miss_q) {
    const uint32_t m = A.mslot[c];
    miss_q[m] = apl::miss_query(cmd);
    miss_get[m] = slot;
  }
}

__global__ void apl_open_seg(lsmck_write_seg* __restrict__ segs, uint64_t g, uint64_t nent) {
  if (blockIdx.x || threadIdx.x) return;
  lsmck_write_seg z;
  z.first_cmd = 0;
  z.first_ent = nent;
  z.mem_bytes = 0;
  segs[g] = z;
}

}  // namespace lsmck

using namespace lsmck;

static int apl_err(hipError_t e) { return e == hipSuccess ? 0 : -(int)e; }
static int apl_launch_err() { return apl_err(hipGetLastError()); }
static unsigned apl_grid(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

extern "C" void lsmk_apl_carve(const MemWs* W, const WplWs* P, AplWs* A) {
  A->ans = W->apos2;
  A->eh = P->ekey;
  A->rs = P->eval;
  A->ew = P->skey;
  A->lw = P->sval;
  A->pq = P->ekey;
  A->gf = P->nxt;
  A->mf = P->exitp;
  A->gslot = P->prev;
  A->mslot = P->skey;
}

extern "C" int lsmk_apl_validate(const lsmck_wal_cmd* cmds, uint64_t n, uint64_t keys_bytes, uint64_t vals_bytes,
                                 const uint8_t* tomb, unsigned long long* info, hipStream_t st) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(apl_validate, dim3(apl_grid(n)), dim3(256), 0, st, cmds, n, keys_bytes, vals_bytes, tomb, info);
  return apl_launch_err();
}

extern "C" int lsmk_apl_prep(const WplWs* Pp, const AplWs* Ap, const lsmck_wal_cmd* cmds, uint64_t n, void* tmp,
                             size_t* tmp_bytes, hipStream_t st) {
  const WplWs& P = *Pp;
  const AplWs& A = *Ap;
  const bool query = tmp == nullptr;
  size_t need = 0, b;
  hipError_t e;
  if (!query) {
    hipLaunchKernelGGL(apl_pack, dim3(apl_grid(n)), dim3(256), 0, st, P, cmds, n);
    if (int rc = apl_launch_err()) return rc;
    hipLaunchKernelGGL(apl_events, dim3(apl_grid(n)), dim3(256), 0, st, P, A, n);
    if (int rc = apl_launch_err()) return rc;
  }
  b = query ? 0 : *tmp_bytes;
  if ((e = rocprim::inclusive_scan(tmp, b, A.eh, A.rs, n, rocprim::maximum<uint32_t>(), st)) != hipSuccess)
    return apl_err(e);
  need = std::max(need, b);
  b = query ? 0 : *tmp_bytes;
  if ((e = rocprim::inclusive_scan(tmp, b, A.ew, A.lw, n, rocprim::maximum<uint32_t>(), st)) != hipSuccess)
    return apl_err(e);
  need = std::max(need, b);
  if (query) {
    *tmp_bytes = std::max<size_t>(need, 1);
    return 0;
  }
  hipLaunchKernelGGL(apl_prev, dim3(apl_grid(n + 1)), dim3(256), 0, st, P, A, n);
  return apl_launch_err();
}

extern "C" int lsmk_apl_flag(const WplWs* Pp, const AplWs* Ap, uint64_t n, unsigned long long* info, void* tmp,
                             size_t* tmp_bytes, hipStream_t st) {
  const WplWs& P = *Pp;
  const AplWs& A = *Ap;
  const bool query = tmp == nullptr;
  size_t need = 0, b;
  hipError_t e;
  if (!query) {
    hipLaunchKernelGGL(apl_clear, dim3(apl_grid(n)), dim3(256), 0, st, P, A, n);
    if (int rc = apl_launch_err()) return rc;
  }
  b = query ? 0 : *tmp_bytes;
  if ((e = rocprim::exclusive_scan(tmp, b, P.act, P.ex, 0u, n + 1, rocprim::plus<uint32_t>(), st)) != hipSuccess)
    return apl_err(e);
  need = std::max(need, b);
  if (!query) {
    hipLaunchKernelGGL(apl_slots, dim3(apl_grid(n)), dim3(256), 0, st, P, A, n);
    if (int rc = apl_launch_err()) return rc;
  }
  b = query ? 0 : *tmp_bytes;
  if ((e = rocprim::exclusive_scan(tmp, b, A.gf, A.gslot, 0u, n, rocprim::plus<uint32_t>(), st)) != hipSuccess)
    return apl_err(e);
  need = std::max(need, b);
  b = query ? 0 : *tmp_bytes;
  if ((e = rocprim::exclusive_scan(tmp, b, A.mf, A.mslot, 0u, n, rocprim::plus<uint32_t>(), st)) != hipSuccess)
    return apl_err(e);
  need = std::max(need, b);
  if (query) {
    *tmp_bytes = std::max<size_t>(need, 1);
    return 0;
  }
  hipLaunchKernelGGL(apl_totals, dim3(1), dim3(64), 0, st, A, n, info);
  return apl_launch_err();
}

extern "C" int lsmk_apl_gets(const WplWs* P, const AplWs* A, const lsmck_wal_cmd* cmds, const uint8_t* vals, uint64_t n,
                             uint64_t tomb_off, lsmck_apply_get* gets, lsmck_get_query* miss_q, uint32_t* miss_get,
                             hipStream_t st) {
  hipLaunchKernelGGL(apl_gets, dim3(apl_grid(n)), dim3(256), 0, st, *P, *A, cmds, vals, n, tomb_off, gets, miss_q,
                     miss_get);
  return apl_launch_err();
}

extern "C" int lsmk_apl_open_seg(lsmck_write_seg* segs, uint64_t g, uint64_t nent, hipStream_t st) {
  hipLaunchKernelGGL(apl_open_seg, dim3(1), dim3(64), 0, st, segs, g, nent);
  return apl_launch_err();
}
