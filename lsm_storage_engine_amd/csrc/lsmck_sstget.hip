// lsmck_sstget.hip -- batch point reads on the GPU (gfx950):
// lsmck_sstable_get_batch, the batch form of SsTable::get
// (src/sync/sstable.rs:97-113, src/tokio/sstable.rs:57-82) over the tables of
// Db::get_internal's loop (src/tokio/db.rs:178-185).  The map's parse, the
// lower bound, the exact hit and the interval scan: lsmck_sstget.h.
//
//   1. get_tab_count: a lane per table checks its spans and finds its index's
//      item count (arithmetic for an index of one key length, else the serial
//      parse); the u64 scan gives every table's place in the item arrays;
//   2. get_items_uniform: a thread per item of a one-length index proves the
//      item in its place; get_items_fill: a lane per other table leaves the
//      item offsets there by the serial parse;
//   3. get_items_keys: a thread per item -- its order key, its position, and
//      its key above its predecessor's;
//   4. get_queries: a thread per query checks it and forms its order key;
//      get_probe, the hot path: a work item per (query, table) pair, table
//      major -- a lower bound over the table's order keys, then the exact
//      hit's record or the interval's walk of headers; a Some lowers the
//      query's winning source (the table's number above a.base: 0 here, the
//      runs in front of the tables for lsmck_db_get_batch) with a vector
//      atomicMin.  A pair whose table lies above the current winner is
//      skipped: that only saves work, the minimum stands however the reads race;
//      -- the error words are read back here, once --
//   5. get_resolve: a thread per query repeats the lookup in its winning table
//      alone and writes the result.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsmck.h"
#include "lsmck_device.h"
#include "lsmck_sstget.h"

namespace lsmck {

// table states
constexpr uint32_t kGetSerial = 0u;   // its items come from the serial parse
constexpr uint32_t kGetUniform = 1u;  // a one-length candidate: its items are proven in parallel
constexpr uint32_t kGetBad = 2u;      // refused: nothing more of it is read

constexpr unsigned long long kGetNo = ~0ull;

// the item scratch holds every table's items (the caller grows it and runs the passes again when it does not)
__device__ __forceinline__ bool get_fits(const GetArgs& a) { return a.itemfirst[a.ntab] <= a.nslots; }

// 1. info[0] = the first table refused
__global__ __launch_bounds__(256) void get_tab_count(GetArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.ntab) return;
  const lsmck_sstable_span s = a.spans[t];
  a.itemfirst[t] = 0;
  a.fail[t] = 0;
  uint64_t c = get::kNo, klen0;
  if (mrg::span_ok(s.data_off, s.data_len, a.data_bytes) && s.data_len <= mrg::kMaxTable &&
      mrg::span_ok(s.index_off, s.index_len, a.index_bytes)) {
    const uint8_t* idx = a.index + s.index_off;
    if (mrg::index_uniform(idx, s.index_len, &c, &klen0)) {
      a.itemfirst[t] = c;
      a.state[t] = kGetUniform;
      return;
    }
    c = get::index_parse(idx, s.index_len, nullptr, 0);
  }
  if (c == get::kNo) {
    atomicMin(a.info, (unsigned long long)t);
    a.state[t] = kGetBad;
    return;
  }
  a.itemfirst[t] = c;
  a.state[t] = kGetSerial;
}

// 2a. a thread per item slot: the items of the one-length candidates
__global__ __launch_bounds__(256) void get_items_uniform(GetArgs a) {
  const uint64_t sl = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (!get_fits(a) || sl >= a.itemfirst[a.ntab]) return;
  const uint64_t t = mrg::table_of(a.itemfirst, a.ntab, sl);
  if (a.state[t] != kGetUniform) return;
  const uint8_t* idx = a.index + a.spans[t].index_off;
  const uint64_t klen0 = mrg::load64(idx + 8u), j = sl - a.itemfirst[t];
  if (get::uniform_item(idx, klen0, j)) a.ioff[sl] = get::uniform_off(klen0, j);
  else atomicOr(a.fail + t, 1u);
}

// 2b. a lane per table whose items are not there yet: the serial parse
__global__ __launch_bounds__(256) void get_items_fill(GetArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.ntab || !get_fits(a)) return;
  const uint64_t k = a.itemfirst[t + 1] - a.itemfirst[t];
  if (a.state[t] == kGetBad || k == 0) return;
  if (a.state[t] == kGetUniform && !(a.fail[t] & 1u)) return;  // (every item checked)
  const lsmck_sstable_span s = a.spans[t];
  if (get::index_parse(a.index + s.index_off, s.index_len, a.ioff + a.itemfirst[t], k) != k) {
    atomicMin(a.info, (unsigned long long)t);
    a.state[t] = kGetBad;
  }
}

// 3. a thread per item slot
__global__ __launch_bounds__(256) void get_items_keys(GetArgs a) {
  const uint64_t sl = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (!get_fits(a) || sl >= a.itemfirst[a.ntab]) return;
  const uint64_t t = mrg::table_of(a.itemfirst, a.ntab, sl);
  if (a.state[t] == kGetBad) return;
  const uint8_t* idx = a.index + a.spans[t].index_off;
  const uint64_t off = a.ioff[sl];
  a.iok[sl] = get::item_okey(idx, off);
  a.ipos[sl] = get::item_pos(idx, off);
  if (sl > a.itemfirst[t] && !get::item_less(idx, a.ioff[sl - 1u], off)) atomicMin(a.info, (unsigned long long)t);
}

// 4a. info[1] = the first query refused
__global__ __launch_bounds__(256) void get_queries(GetArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const lsmck_get_query q = a.q[i];
  mrg::OKey k;
  k.chunk = 0, k.tail = 0, k.klen = 0;
  if (get::query_ok(q, a.qkeys_bytes)) k = get::key_of(a.qkeys, q.key_off, q.klen).ok;
  else atomicMin(a.info + 1, (unsigned long long)i);
  a.qok[i] = k;
  a.win[i] = get::kNoTable;
}

// 4b. the (query, table) pairs, table major: pair w = t * n + i
__global__ __launch_bounds__(256) void get_probe(GetArgs a) {
  if (a.info[0] != kGetNo || a.info[1] != kGetNo || !get_fits(a)) return;  // (the call fails: nothing is looked up)
  const uint64_t total = a.n * a.ntab, stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += stride) {
    const uint64_t t = w / a.n, i = w - t * a.n;
    if (a.base + t > __atomic_load_n(a.win + i, __ATOMIC_RELAXED)) continue;  // (a lower source answered already)
    const get::Table T = get::table_at(a, t);
    const get::Key k = get::key_at(a, i);
    uint64_t vpos;
    uint32_t vlen;
    bool walked;
    if (get::table_get(T, k, &vpos, &vlen, &walked)) atomicMin(a.win + i, (uint32_t)(a.base + t));
    if (a.count) {
      atomicAdd(a.info + 3, 1ull);
      if (walked) atomicAdd(a.info + 4, 1ull);
    }
  }
}

// 5. a thread per query
__global__ __launch_bounds__(256) void get_resolve(GetArgs a, lsmck_get_result* __restrict__ res) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t t = a.win[i];
  lsmck_get_result r = get::result_none();
  if (t != get::kNoTable) {
    const get::Table T = get::table_at(a, t);
    uint64_t vpos;
    uint32_t vlen;
    if (get::table_get(T, get::key_at(a, i), &vpos, &vlen, nullptr))
      r = get::result_of(T.img, a.spans[t].data_off, vpos, vlen, t);
  }
  res[i] = r;
}

}  // namespace lsmck

using namespace lsmck;

static int get_launch_err() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
static unsigned get_grid(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

extern "C" int lsmk_get_index(const lsmck::GetArgs* a, hipStream_t st) {
  hipLaunchKernelGGL(get_tab_count, dim3(get_grid(a->ntab)), dim3(256), 0, st, *a);
  int rc = lsmk_sst_scan(a->itemfirst, a->ntab, a->bsum, a->info + 2, st);
  if (rc || !a->nslots) return rc;
  hipLaunchKernelGGL(get_items_uniform, dim3(get_grid(a->nslots)), dim3(256), 0, st, *a);
  hipLaunchKernelGGL(get_items_fill, dim3(get_grid(a->ntab)), dim3(256), 0, st, *a);
  hipLaunchKernelGGL(get_items_keys, dim3(get_grid(a->nslots)), dim3(256), 0, st, *a);
  return get_launch_err();
}
extern "C" int lsmk_get_queries(const lsmck::GetArgs* a, hipStream_t st) {
  hipLaunchKernelGGL(get_queries, dim3(get_grid(a->n)), dim3(256), 0, st, *a);
  return get_launch_err();
}
extern "C" int lsmk_get_pairs(const lsmck::GetArgs* a, hipStream_t st) {
  if (a->ntab) {
    // at most 2^20 workgroups; the pairs beyond them by the grid's stride
    const uint64_t blocks = (a->n * a->ntab + 255u) / 256u;
    hipLaunchKernelGGL(get_probe, dim3((unsigned)(blocks < (1ull << 20) ? blocks : (1ull << 20))), dim3(256), 0, st, *a);
  }
  return get_launch_err();
}
extern "C" int lsmk_get_probe(const lsmck::GetArgs* a, hipStream_t st) {
  const int rc = lsmk_get_queries(a, st);
  return rc ? rc : lsmk_get_pairs(a, st);
}
extern "C" int lsmk_get_resolve(const lsmck::GetArgs* a, lsmck_get_result* res, hipStream_t st) {
  hipLaunchKernelGGL(get_resolve, dim3(get_grid(a->n)), dim3(256), 0, st, *a, res);
  return get_launch_err();
}
