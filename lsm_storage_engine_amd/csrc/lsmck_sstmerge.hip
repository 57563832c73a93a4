// lsmck_sstmerge.hip -- batch SSTable decode and compaction merge on the GPU
// (gfx950): lsmck_sstable_decode_batch and lsmck_sstable_merge_batch, the
// batch forms of the data file's iterator (src/sync/sstable.rs:77-90,
// datafile.rs:60-83) and of SsTable::merge_compact's loop
// (src/sync/sstable.rs:171-208).  The record step, the index parse, the hint's
// acceptance rule, the order keys and the rank rules: lsmck_sstmerge.h.
//
// Decode (dec_*):
//   1. dec_index_count: a lane per table checks its spans and, with an index,
//      parses the index image: the items it would add to the hint;
//      the u64 scan gives every table's place in the segment scratch;
//   2. dec_index_uniform: a thread per item of an index whose keys have one
//      length proves the item in its place (no serial parse for such a table);
//      dec_index_fill: a lane per other table leaves the segment starts there;
//   3. dec_seg_check: a thread per segment walks at most 100 headers and
//      checks its landing; a table's last segment leaves its record count;
//   4. dec_count: a lane per table -- a table whose hint stood is counted from
//      its segments, any other one is walked plainly; the u64 scan gives the
//      tables' first entry numbers;
//      -- the total and the error word are read back here, once --
//   5. dec_emit_seg / dec_emit_plain: the entries.
// Merge (mrg_*):
//   1. mrg_okey: every entry's validity, order key and table; mrg_order: every
//      table strictly increasing;
//   2. mrg_shadow: a thread per entry looks for its key in the newer tables of
//      its group; live flags (u64, the scan's input) and tombstone winners;
//   3. the u64 scan of the live flags; mrg_stuck: the first tombstone winner in
//      (group, key) order; mrg_groups: the groups' first output entries;
//      -- the count and the error words are read back here, once --
//   4. mrg_place: a thread per live entry computes its slot and writes it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsmck.h"
#include "lsmck_device.h"
#include "lsmck_sstmerge.h"

namespace lsmck {

// table states of the decode
constexpr uint32_t kDecHint = 0u;      // the index is a candidate hint
constexpr uint32_t kDecDeclined = 1u;  // an index was given and refused: walked plainly, counted
constexpr uint32_t kDecPlain = 2u;     // no index, or spans out of range: walked plainly (or not at all)
constexpr uint32_t kDecUniform = 3u;   // a candidate hint whose items are proven in parallel (mrg::index_uniform)
__device__ __forceinline__ bool dec_is_hint(uint32_t s) { return s == kDecHint || s == kDecUniform; }

// 1. info[0] = the first table whose spans are refused
__global__ __launch_bounds__(256) void dec_index_count(const uint8_t* __restrict__ data, uint64_t data_bytes,
                                                        const uint8_t* __restrict__ index, uint64_t index_bytes,
                                                        const lsmck_sstable_span* __restrict__ spans, uint64_t ntab,
                                                        uint64_t* __restrict__ nseg, uint32_t* __restrict__ state,
                                                        uint32_t* __restrict__ fail,
                                                        unsigned long long* __restrict__ info) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntab) return;
  const lsmck_sstable_span s = spans[t];
  nseg[t] = 0;
  fail[t] = 0;
  bool ok = mrg::span_ok(s.data_off, s.data_len, data_bytes) && s.data_len <= mrg::kMaxTable;
  if (index) ok = ok && mrg::span_ok(s.index_off, s.index_len, index_bytes);
  if (!ok) {
    atomicMin(info, (unsigned long long)t);
    state[t] = kDecPlain;
    fail[t] = 2u;  // (nothing of this table is read)
    return;
  }
  if (!index) {
    state[t] = kDecPlain;
    return;
  }
  uint64_t c, klen0;
  if (mrg::index_uniform(index + s.index_off, s.index_len, &c, &klen0)) {
    nseg[t] = c;
    state[t] = kDecUniform;
    return;
  }
  c = mrg::index_parse(index + s.index_off, s.index_len, s.data_len, nullptr, 0);
  if (c == ~0ull) {
    state[t] = kDecDeclined;
  } else if (c == 0) {
    state[t] = mrg::empty_check(data + s.data_off, s.data_len) ? kDecHint : kDecDeclined;
  } else {
    nseg[t] = c;
    state[t] = kDecHint;
  }
}

// 2a. a thread per item of the uniform candidates: the item proven in its
// place, its position to segpos; a table with an item that does not check is
// parsed serially below
__global__ __launch_bounds__(256) void dec_index_uniform(const uint8_t* __restrict__ index,
                                                          const lsmck_sstable_span* __restrict__ spans, uint64_t ntab,
                                                          const uint64_t* __restrict__ segfirst, uint64_t nslots,
                                                          uint64_t* __restrict__ segpos,
                                                          const uint32_t* __restrict__ state,
                                                          uint32_t* __restrict__ fail) {
  const uint64_t sl = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (sl >= nslots || sl >= segfirst[ntab]) return;
  const uint64_t t = mrg::table_of(segfirst, ntab, sl);
  if (state[t] != kDecUniform) return;
  const lsmck_sstable_span s = spans[t];
  const uint8_t* idx = index + s.index_off;
  uint64_t p;
  if (mrg::uniform_item(idx, s.data_len, mrg::load64(idx + 8u), sl - segfirst[t], &p)) segpos[sl] = p;
  else atomicOr(fail + t, 1u);
}

// 2b. the segment starts of table t at segpos[segfirst[t] ..] by the serial
// parse; a table whose items do not fit the scratch (overlapping index spans)
// is declined
__global__ __launch_bounds__(256) void dec_index_fill(const uint8_t* __restrict__ index,
                                                       const lsmck_sstable_span* __restrict__ spans, uint64_t ntab,
                                                       const uint64_t* __restrict__ segfirst, uint64_t nslots,
                                                       uint64_t* __restrict__ segpos, uint32_t* __restrict__ state,
                                                       uint32_t* __restrict__ fail,
                                                       unsigned long long* __restrict__ info) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntab) return;
  const uint64_t k = segfirst[t + 1] - segfirst[t];
  if (!dec_is_hint(state[t]) || k == 0) return;
  if (segfirst[t + 1] > nslots) {
    state[t] = kDecDeclined;
    return;
  }
  if (state[t] == kDecUniform) {
    if (!(fail[t] & 1u)) {  // (every item checked)
      atomicAdd(info + 4, 1ull);
      return;
    }
    fail[t] = 0;
  }
  const lsmck_sstable_span s = spans[t];
  if (mrg::index_parse(index + s.index_off, s.index_len, s.data_len, segpos + segfirst[t], k) != k)
    state[t] = kDecDeclined;
}

// 3. a thread per segment slot
__global__ __launch_bounds__(256) void dec_seg_check(const uint8_t* __restrict__ data,
                                                      const lsmck_sstable_span* __restrict__ spans, uint64_t ntab,
                                                      const uint64_t* __restrict__ segfirst, uint64_t nslots,
                                                      const uint64_t* __restrict__ segpos,
                                                      const uint32_t* __restrict__ state, uint32_t* __restrict__ fail,
                                                      uint32_t* __restrict__ lastcnt, uint64_t* __restrict__ cons) {
  const uint64_t sl = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (sl >= nslots || sl >= segfirst[ntab]) return;
  const uint64_t t = mrg::table_of(segfirst, ntab, sl);
  if (!dec_is_hint(state[t])) return;
  const lsmck_sstable_span s = spans[t];
  const bool last = sl + 1u == segfirst[t + 1];
  uint32_t c;
  uint64_t end;
  if (!mrg::seg_check(data + s.data_off, s.data_len, segpos[sl], last, last ? 0 : segpos[sl + 1u], &c, &end)) {
    atomicOr(fail + t, 1u);
  } else if (last) {
    lastcnt[t] = c;
    cons[t] = end;
  }
}

// 4. cnt[t] = table t's entries, cons[t] = the bytes its iterator got through,
// hint[t] = its entries come from the segments; info[2] counts the tables
// whose index was refused
__global__ __launch_bounds__(64) void dec_count(const uint8_t* __restrict__ data,
                                                 const lsmck_sstable_span* __restrict__ spans, uint64_t ntab,
                                                 const uint64_t* __restrict__ segfirst,
                                                 const uint32_t* __restrict__ state, const uint32_t* __restrict__ fail,
                                                 const uint32_t* __restrict__ lastcnt, uint64_t* __restrict__ cons,
                                                 uint64_t* __restrict__ cnt, uint8_t* __restrict__ hint,
                                                 unsigned long long* __restrict__ info) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntab) return;
  hint[t] = 0;
  if (fail[t] & 2u) {  // (its spans were refused)
    cnt[t] = 0, cons[t] = 0;
    return;
  }
  const uint64_t k = segfirst[t + 1] - segfirst[t];
  if (dec_is_hint(state[t]) && !fail[t]) {
    hint[t] = 1;
    cnt[t] = k ? (k - 1u) * mrg::kStep + lastcnt[t] : 0u;
    if (!k) cons[t] = 0;
    return;
  }
  if (state[t] != kDecPlain) atomicAdd(info + 2, 1ull);
  const lsmck_sstable_span s = spans[t];
  uint64_t end;
  cnt[t] = mrg::walk(data + s.data_off, s.data_len, s.data_off, 0, ~0ull, nullptr, &end);
  cons[t] = end;
}

// 5. the entries
__global__ __launch_bounds__(256) void dec_emit_seg(const uint8_t* __restrict__ data,
                                                     const lsmck_sstable_span* __restrict__ spans, uint64_t ntab,
                                                     const uint64_t* __restrict__ segfirst, uint64_t nslots,
                                                     const uint64_t* __restrict__ segpos,
                                                     const uint8_t* __restrict__ hint,
                                                     const uint64_t* __restrict__ tabfirst,
                                                     lsmck_wal_cmd* __restrict__ ents) {
  const uint64_t sl = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (sl >= nslots || sl >= segfirst[ntab]) return;
  const uint64_t t = mrg::table_of(segfirst, ntab, sl);
  if (!hint[t]) return;
  const lsmck_sstable_span s = spans[t];
  // (the check bounds the walk: kStep records, the last segment tabfirst[t + 1] - its first entry)
  const uint64_t e0 = tabfirst[t] + (sl - segfirst[t]) * mrg::kStep;
  const uint64_t room = tabfirst[t + 1] - e0;
  uint64_t end;
  (void)mrg::walk(data + s.data_off, s.data_len, s.data_off, segpos[sl], room < mrg::kStep ? room : mrg::kStep,
                  ents + e0, &end);
}
__global__ __launch_bounds__(64) void dec_emit_plain(const uint8_t* __restrict__ data,
                                                      const lsmck_sstable_span* __restrict__ spans, uint64_t ntab,
                                                      const uint8_t* __restrict__ hint,
                                                      const uint64_t* __restrict__ tabfirst,
                                                      lsmck_wal_cmd* __restrict__ ents) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntab || hint[t]) return;
  const lsmck_sstable_span s = spans[t];
  uint64_t end;
  (void)mrg::walk(data + s.data_off, s.data_len, s.data_off, 0, tabfirst[t + 1] - tabfirst[t], ents + tabfirst[t], &end);
}

// ---- merge ------------------------------------------------------------------

// 1. info[0] = the first entry refused
__global__ __launch_bounds__(256) void mrg_okey(const lsmck_wal_cmd* __restrict__ ents, uint64_t n,
                                                 const uint8_t* __restrict__ keys, uint64_t kb, uint64_t vb,
                                                 const uint64_t* __restrict__ tf, uint64_t ntab,
                                                 mrg::OKey* __restrict__ ok, uint32_t* __restrict__ etab,
                                                 unsigned long long* __restrict__ info) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const lsmck_wal_cmd c = ents[i];
  etab[i] = (uint32_t)mrg::table_of(tf, ntab, i);
  mrg::OKey k;
  k.chunk = 0, k.tail = 0, k.klen = 0;
  if (sst::rec_size(c, kb, vb)) k = mrg::okey_of(keys, c);
  else atomicMin(info, (unsigned long long)i);
  ok[i] = k;
}
// a thread per entry that is not its table's first: its key against its
// predecessor's (sst_order's rule; entries refused above are reported already)
__global__ __launch_bounds__(256) void mrg_order(const lsmck_wal_cmd* __restrict__ ents, uint64_t n,
                                                  const uint8_t* __restrict__ keys, uint64_t kb, uint64_t vb,
                                                  const uint32_t* __restrict__ etab,
                                                  unsigned long long* __restrict__ info) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + 1u;
  if (i >= n || etab[i] != etab[i - 1]) return;
  const lsmck_wal_cmd a = ents[i - 1], b = ents[i];
  if (!sst::rec_size(a, kb, vb) || !sst::rec_size(b, kb, vb)) return;
  if (!sst::key_less(keys + a.key_off, a.klen, keys + b.key_off, b.klen)) atomicMin(info, (unsigned long long)i);
}

// 2. live[i] = 1 for a winner that stays; tomb[i] = 1 for a tombstone winner
// in the mode that reports it.  mode: 0 report, 1 drop, 2 keep.
__global__ __launch_bounds__(256) void mrg_shadow(const lsmck_wal_cmd* __restrict__ ents, uint64_t n,
                                                   const uint8_t* __restrict__ keys, const uint8_t* __restrict__ vals,
                                                   const uint64_t* __restrict__ tf, const uint64_t* __restrict__ gf,
                                                   const uint32_t* __restrict__ tgrp, const mrg::OKey* __restrict__ ok,
                                                   const uint32_t* __restrict__ etab, uint32_t mode,
                                                   uint64_t* __restrict__ live, uint8_t* __restrict__ tomb,
                                                   const unsigned long long* __restrict__ info) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (info[0] != ~0ull) {  // (a refused entry: the call fails, and no key of it is read)
    live[i] = 0, tomb[i] = 0;
    return;
  }
  const uint64_t t = etab[i];
  const bool sh = mrg::shadowed(ok, ents, keys, tf, t, gf[tgrp[t] + 1u], i);
  const bool tb = !sh && mode != 2u && mrg::tombstone(ents[i], vals);
  live[i] = !sh && !(tb && mode == 1u);
  tomb[i] = tb && mode == 0u;
}

// 3. info[2] = the first tombstone winner in (group, key) order: its slot
// among the winners in the high word, the entry in the low one
__global__ __launch_bounds__(256) void mrg_stuck(const lsmck_wal_cmd* __restrict__ ents, uint64_t n,
                                                  const uint8_t* __restrict__ keys, const uint64_t* __restrict__ tf,
                                                  const uint64_t* __restrict__ gf, const uint32_t* __restrict__ tgrp,
                                                  const mrg::OKey* __restrict__ ok, const uint32_t* __restrict__ etab,
                                                  const uint64_t* __restrict__ lp, const uint8_t* __restrict__ tomb,
                                                  unsigned long long* __restrict__ info) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !tomb[i]) return;
  const uint64_t t = etab[i], g = tgrp[t];
  const uint64_t slot = mrg::slot_of(ok, ents, keys, tf, lp, gf[g], gf[g + 1u], t, i);
  atomicMin(info + 2, (unsigned long long)((slot << 32) | i));
}
__global__ __launch_bounds__(256) void mrg_groups(const uint64_t* __restrict__ tf, const uint64_t* __restrict__ gf,
                                                   uint64_t ngrp, const uint64_t* __restrict__ lp,
                                                   uint64_t* __restrict__ gout) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g <= ngrp) gout[g] = lp[tf[gf[g]]];
}

// 4. a thread per live entry
__global__ __launch_bounds__(256) void mrg_place(const lsmck_wal_cmd* __restrict__ ents, uint64_t n,
                                                  const uint8_t* __restrict__ keys, const uint64_t* __restrict__ tf,
                                                  const uint64_t* __restrict__ gf, const uint32_t* __restrict__ tgrp,
                                                  const mrg::OKey* __restrict__ ok, const uint32_t* __restrict__ etab,
                                                  const uint64_t* __restrict__ lp, lsmck_wal_cmd* __restrict__ out,
                                                  uint32_t* __restrict__ src) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || lp[i + 1u] == lp[i]) return;
  const uint64_t t = etab[i], g = tgrp[t];
  const uint64_t slot = mrg::slot_of(ok, ents, keys, tf, lp, gf[g], gf[g + 1u], t, i);
  lsmck_wal_cmd c = ents[i];
  c.reserved = 0;
  out[slot] = c;
  if (src) src[slot] = (uint32_t)i;
}

}  // namespace lsmck

using namespace lsmck;

static int mrg_launch_err() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
static unsigned mrg_grid(uint64_t n, unsigned block = 256u) { return (unsigned)((n + block - 1u) / block); }

extern "C" int lsmk_dec_index(const lsmck::DecArgs* a, hipStream_t st) {
  hipLaunchKernelGGL(dec_index_count, dim3(mrg_grid(a->ntab)), dim3(256), 0, st, a->data, a->data_bytes, a->index,
                     a->index_bytes, a->spans, a->ntab, a->segfirst, a->state, a->fail, a->info);
  int rc = lsmk_sst_scan(a->segfirst, a->ntab, a->bsum, a->info + 3, st);
  if (rc || !a->index) return rc;
  hipLaunchKernelGGL(dec_index_uniform, dim3(mrg_grid(a->nslots)), dim3(256), 0, st, a->index, a->spans, a->ntab,
                     (const uint64_t*)a->segfirst, a->nslots, a->segpos, (const uint32_t*)a->state, a->fail);
  hipLaunchKernelGGL(dec_index_fill, dim3(mrg_grid(a->ntab)), dim3(256), 0, st, a->index, a->spans, a->ntab,
                     (const uint64_t*)a->segfirst, a->nslots, a->segpos, a->state, a->fail, a->info);
  return mrg_launch_err();
}
extern "C" int lsmk_dec_segments(const lsmck::DecArgs* a, hipStream_t st) {
  if (!a->index || !a->nslots) return 0;
  hipLaunchKernelGGL(dec_seg_check, dim3(mrg_grid(a->nslots)), dim3(256), 0, st, a->data, a->spans, a->ntab,
                     (const uint64_t*)a->segfirst, a->nslots, (const uint64_t*)a->segpos, (const uint32_t*)a->state,
                     a->fail, a->lastcnt, a->cons);
  return mrg_launch_err();
}
extern "C" int lsmk_dec_count(const lsmck::DecArgs* a, hipStream_t st) {
  hipLaunchKernelGGL(dec_count, dim3(mrg_grid(a->ntab, 64u)), dim3(64), 0, st, a->data, a->spans, a->ntab,
                     (const uint64_t*)a->segfirst, (const uint32_t*)a->state, (const uint32_t*)a->fail,
                     (const uint32_t*)a->lastcnt, a->cons, a->tabfirst, a->hint, a->info);
  return lsmk_sst_scan(a->tabfirst, a->ntab, a->bsum, a->info + 1, st);
}
extern "C" int lsmk_dec_emit(const lsmck::DecArgs* a, lsmck_wal_cmd* ents, hipStream_t st) {
  if (a->index && a->nslots)
    hipLaunchKernelGGL(dec_emit_seg, dim3(mrg_grid(a->nslots)), dim3(256), 0, st, a->data, a->spans, a->ntab,
                       (const uint64_t*)a->segfirst, a->nslots, (const uint64_t*)a->segpos, (const uint8_t*)a->hint,
                       (const uint64_t*)a->tabfirst, ents);
  hipLaunchKernelGGL(dec_emit_plain, dim3(mrg_grid(a->ntab, 64u)), dim3(64), 0, st, a->data, a->spans, a->ntab,
                     (const uint8_t*)a->hint, (const uint64_t*)a->tabfirst, ents);
  return mrg_launch_err();
}

extern "C" int lsmk_mrg_keys(const lsmck::MrgArgs* a, hipStream_t st) {
  hipLaunchKernelGGL(mrg_okey, dim3(mrg_grid(a->n)), dim3(256), 0, st, a->ents, a->n, a->keys, a->keys_bytes,
                     a->vals_bytes, a->tf, a->ntab, a->ok, a->etab, a->info);
  if (a->n > 1)
    hipLaunchKernelGGL(mrg_order, dim3(mrg_grid(a->n - 1)), dim3(256), 0, st, a->ents, a->n, a->keys, a->keys_bytes,
                       a->vals_bytes, (const uint32_t*)a->etab, a->info);
  return mrg_launch_err();
}
extern "C" int lsmk_mrg_shadow(const lsmck::MrgArgs* a, hipStream_t st) {
  hipLaunchKernelGGL(mrg_shadow, dim3(mrg_grid(a->n)), dim3(256), 0, st, a->ents, a->n, a->keys, a->vals, a->tf, a->gf,
                     a->tgrp, (const mrg::OKey*)a->ok, (const uint32_t*)a->etab, a->mode, a->live, a->tomb,
                     (const unsigned long long*)a->info);
  return mrg_launch_err();
}
extern "C" int lsmk_mrg_scan(const lsmck::MrgArgs* a, hipStream_t st) {
  int rc = lsmk_sst_scan(a->live, a->n, a->bsum, a->info + 1, st);
  if (rc) return rc;
  if (a->mode == 0u)
    hipLaunchKernelGGL(mrg_stuck, dim3(mrg_grid(a->n)), dim3(256), 0, st, a->ents, a->n, a->keys, a->tf, a->gf, a->tgrp,
                       (const mrg::OKey*)a->ok, (const uint32_t*)a->etab, (const uint64_t*)a->live,
                       (const uint8_t*)a->tomb, a->info);
  hipLaunchKernelGGL(mrg_groups, dim3(mrg_grid(a->ngrp + 1)), dim3(256), 0, st, a->tf, a->gf, a->ngrp,
                     (const uint64_t*)a->live, a->gout);
  return mrg_launch_err();
}
extern "C" int lsmk_mrg_place(const lsmck::MrgArgs* a, lsmck_wal_cmd* out, uint32_t* src, hipStream_t st) {
  hipLaunchKernelGGL(mrg_place, dim3(mrg_grid(a->n)), dim3(256), 0, st, a->ents, a->n, a->keys, a->tf, a->gf, a->tgrp,
                     (const mrg::OKey*)a->ok, (const uint32_t*)a->etab, (const uint64_t*)a->live, out, src);
  return mrg_launch_err();
}
