// lsmck_dbget.hip -- batch Db::get on the GPU (gfx950): lsmck_db_get_batch,
// Db::get (src/tokio/db.rs:144-189) for many keys over runs -- the memtable
// and the old memtable as sorted entries -- in front of the tables of
// lsmck_sstable_get_batch, the values gathered into one packed arena.  What
// decides a result: lsmck_dbget.h, and lsmck_sstget.h for the tables.
//
//   1. dbg_run_pass: a thread per entry of all runs -- its rule, its order
//      key, its key above its predecessor's in its run;
//   2. the point read's index pass and query check (lsmck_sstget.hip);
//   3. dbg_probe: a work item per (query, run) pair, run major -- a lower
//      bound over the run's order keys; a hit lowers the query's winning
//      source with a vector atomicMin.  It ends before the table probe
//      starts, so a key a run answered costs that probe one load;
//   4. the point read's table probe, its tables numbered from nrun;
//   5. dbg_resolve: a thread per query repeats the lookup in its winning
//      source alone and leaves the result, the answered length and the
//      value's address in scratch; the u64 scan of the lengths;
//      -- the error words and the total are read back here, once --
//   6. dbg_gather, the hot path that is new: a workgroup per 32 KiB of `out`.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsmck.h"
#include "lsmck_device.h"
#include "lsmck_dbget.h"

namespace lsmck {

constexpr unsigned long long kDbgNo = ~0ull;

// the call fails: nothing more is looked up (a refused entry's ranges may lie anywhere)
__device__ __forceinline__ bool dbg_failed(const DbArgs& a) {
  return a.g.info[0] != kDbgNo || a.g.info[1] != kDbgNo || a.g.info[5] != kDbgNo;
}

// 1. info[5] = the first run entry refused, counted across the runs
__global__ __launch_bounds__(256) void dbg_run_pass(DbArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.nent) return;
  if (!dbg::run_pass(a.runs, a.rf, a.nrun, e, a.rok)) atomicMin(a.g.info + 5, (unsigned long long)e);
}

__device__ __forceinline__ dbg::Run dbg_run(const DbArgs& a, uint64_t r) { return dbg::run_of(a.runs[r], a.rok + a.rf[r]); }

// 3. the (query, run) pairs, run major: pair w = r * n + i
__global__ __launch_bounds__(256) void dbg_probe(DbArgs a) {
  if (dbg_failed(a)) return;
  const uint64_t total = a.g.n * a.nrun, stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += stride) {
    const uint64_t r = w / a.g.n, i = w - r * a.g.n;
    if (r > __atomic_load_n(a.g.win + i, __ATOMIC_RELAXED)) continue;  // (a lower run answered already)
    uint64_t at;
    if (dbg::run_get(dbg_run(a, r), get::key_at(a.g, i), &at)) atomicMin(a.g.win + i, (uint32_t)r);
  }
}

// 5. a thread per query
__global__ __launch_bounds__(256) void dbg_resolve(DbArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.g.n) return;
  lsmck_get_result x = get::result_none();
  uint64_t src = 0;
  // (a call that fails, or whose item scratch has to grow, leaves no result: the lengths then add up to 0)
  if (!dbg_failed(a) && (!a.g.ntab || a.g.itemfirst[a.g.ntab] <= a.g.nslots)) {
    const uint32_t s = a.g.win[i];
    if (s < a.nrun) {
      const dbg::Run R = dbg_run(a, s);
      uint64_t at;
      if (dbg::run_get(R, get::key_at(a.g, i), &at)) {
        const lsmck_wal_cmd c = R.ents[at];
        x = dbg::run_result(R, c, s);
        src = (uint64_t)(uintptr_t)(R.vals + c.val_off);
        if (a.g.count) atomicAdd(a.g.info + 6, 1ull);
      }
    } else if (s != get::kNoTable) {
      const uint64_t t = s - a.nrun;
      const get::Table T = get::table_at(a.g, t);
      uint64_t vpos;
      uint32_t vlen;
      if (get::table_get(T, get::key_at(a.g, i), &vpos, &vlen, nullptr)) {
        x = get::result_of(T.img, a.g.spans[t].data_off, vpos, vlen, s);
        src = (uint64_t)(uintptr_t)(T.img + vpos);
      }
    }
  }
  a.res[i] = x;
  if (a.len) {
    a.len[i] = dbg::answered_len(x);
    a.src[i] = src;
  }
}

// 6. The gather (lsmck_dbget.h): a workgroup per tile, 256 consecutive chunks
// per pass of the block.  The tile's first value comes from the search of
// off[] by the whole wave (enc::probe / narrow), made by each of the four
// waves for itself; the offsets of the values that start inside the tile then
// go to LDS, relative to the tile (u16), a block's load at a time until one
// ends past the tile, and with them the addresses of the tile's first 256
// values.  A tile in which more than kSlice values start -- zero-length ones
// start no byte -- searches off[] itself.
__global__ __launch_bounds__(dbg::kBlock) void dbg_gather(const uint64_t* __restrict__ off,
                                                           const uint64_t* __restrict__ src, uint64_t n,
                                                           uint8_t* __restrict__ out) {
  __shared__ dbg::slice_t srel[dbg::kSlice + 1u];
  __shared__ uint64_t cache[dbg::kCache];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  dbg::Tile t;
  t.off = off, t.src = src, t.n = n;
  t.total = (int64_t)off[n];
  // (the first tile starts at or before out: ts <= 0)
  t.ts = (int64_t)blockIdx.x * dbg::kTile - (int64_t)((uintptr_t)out & (dbg::kTile - 1u));
  const int64_t t0 = t.ts > 0 ? t.ts : 0;
  uint64_t lo = 0, hi = n;  // off[0] = 0 <= t0 < total = off[n]
  while (hi - lo > 1) {     // (wave-uniform; among equal offsets the last one is found: it owns the byte)
    const uint64_t idx = enc::probe(lo, hi, lane);
    const bool le = idx < hi && (int64_t)off[idx] <= t0;
    enc::narrow(lo, hi, (uint32_t)__popcll(__ballot(le)));
  }
  t.r0 = lo;
  t.off0 = (int64_t)off[lo];
  if (tid == 0) srel[0] = 0;
  if (t.r0 + tid < n) cache[tid] = src[t.r0 + tid];
  t.N = 1;
  bool whole = false;  // the slice holds every value that starts inside the tile
  for (uint32_t base = 0; base < dbg::kSlice; base += dbg::kBlock) {
    const uint32_t v = dbg::slice_entry(off, n, t.r0, 1u + base + tid, t.ts);
    srel[1u + base + tid] = (dbg::slice_t)v;
    t.N += dbg::kBlock;
    if (!__syncthreads_or(tid == dbg::kBlock - 1u && v < dbg::kTile)) {  // (the load's last entry is past the tile)
      whole = true;
      break;
    }
  }
  if (whole) {
    dbg::Slice rel;
    rel.s = srel;
    for (uint32_t p = tid * 16u; p < dbg::kTile; p += dbg::kGroup * dbg::kBlock * 16u)
      dbg::chunks(t, rel, (const uint64_t*)cache, p, dbg::kBlock * 16u, out);
  } else {
    t.N = n - t.r0 + 1u;  // (every offset from off[r0] to off[n])
    for (uint32_t p = tid * 16u; p < dbg::kTile; p += dbg::kGroup * dbg::kBlock * 16u)
      dbg::chunks(t, dbg::Global(), (const uint64_t*)cache, p, dbg::kBlock * 16u, out);
  }
}

}  // namespace lsmck

using namespace lsmck;

static int dbg_launch_err() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
static unsigned dbg_grid(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

extern "C" int lsmk_dbg_runs(const lsmck::DbArgs* a, hipStream_t st) {
  hipLaunchKernelGGL(dbg_run_pass, dim3(dbg_grid(a->nent)), dim3(256), 0, st, *a);
  return dbg_launch_err();
}
extern "C" int lsmk_dbg_probe(const lsmck::DbArgs* a, hipStream_t st) {
  // at most 2^20 workgroups; the pairs beyond them by the grid's stride
  const uint64_t blocks = (a->g.n * a->nrun + 255u) / 256u;
  hipLaunchKernelGGL(dbg_probe, dim3((unsigned)(blocks < (1ull << 20) ? blocks : (1ull << 20))), dim3(256), 0, st, *a);
  return dbg_launch_err();
}
extern "C" int lsmk_dbg_resolve(const lsmck::DbArgs* a, hipStream_t st) {
  hipLaunchKernelGGL(dbg_resolve, dim3(dbg_grid(a->g.n)), dim3(256), 0, st, *a);
  const int rc = dbg_launch_err();
  if (rc || !a->len) return rc;
  return lsmk_sst_scan(a->len, a->g.n, a->g.bsum, a->g.info + 7, st);
}
extern "C" int lsmk_dbg_gather(const lsmck::DbArgs* a, uint8_t* out, uint64_t total, hipStream_t st) {
  if (a->g.n == 0 || total == 0) return 0;
  const uint64_t tiles = (((uintptr_t)out & (dbg::kTile - 1u)) + total + dbg::kTile - 1u) / dbg::kTile;
  if (tiles > 0x7FFFFFFFull) return -(int)hipErrorInvalidValue;
  hipLaunchKernelGGL(dbg_gather, dim3((unsigned)tiles), dim3(dbg::kBlock), 0, st, (const uint64_t*)a->len,
                     (const uint64_t*)a->src, a->g.n, out);
  return dbg_launch_err();
}
