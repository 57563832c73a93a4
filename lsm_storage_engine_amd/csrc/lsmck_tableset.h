// lsmck_tableset.h -- the opened table set (lsmck_tableset_open,
// lsmck_tableset_get_batch): the per-table key fences, which the kernels
// (lsmck_tableset.hip ts_*) and the host model that runs the same code under a
// sanitizer (tests/native/test_tableset.cpp) share.  Internal to liblsmck.so.
//
// A set keeps what the point read's index pass proves (lsmck_sstget.h: per
// item an order key, its offset in the index image and its position) between
// calls, and per table two fences.  A fence is a key with a proof: every query
// on its far side is None under the literal SsTable::get
// (src/tokio/sstable.rs:57-82), whatever the table's bytes are.  For a table
// with items (key_j, pos_j), j < m, and data length L:
//   * low (m >= 1): the walk of scan_range(0, pos_0) -- the record at 0 is
//     attempted even when pos_0 is 0, then the walk goes on while pos < pos_0
//     and a whole record fits.  Valid when it ends within `cap` records and no
//     visited key is below key_0.  A query k < key_0 has no item below it and
//     key_0 as the first above: get scans exactly that walk and finds only
//     keys >= key_0 > k.
//   * high (m >= 1): the walk of scan_range(pos_{m-1}, L).  Valid when it ends
//     within `cap` records; hi = max(key_{m-1}, the visited keys).  A query
//     k > hi lies above every item: get scans exactly that walk and finds only
//     keys <= hi < k.
//   * m == 0: none (every query walks from 0 to L).
// Positions may be any u64, the record at an item's position may hold any
// key, tails may be unsorted or end in a cut record: nothing above assumes a
// well-formed table.  Compares take the order keys first and read key bytes
// only on a tie past 8 bytes, as get::item_cmp does.
#ifndef LSMCK_TABLESET_H
#define LSMCK_TABLESET_H
#include <stdint.h>

#include "lsmck.h"
#include "lsmck_sstget.h"

namespace lsmck {
namespace ts {

constexpr uint32_t kWalkCap = 256u;  // "fence_walk_cap": INDEX_STEP is 100, an interval with one item missing 200

// a fence's key: its order key, its length and where its bytes lie (an item's
// key in the index image, or a record's in the data image)
struct FKey {
  mrg::OKey ok;
  uint64_t klen;
  const uint8_t* p;
};
constexpr uint32_t kLow = 1u, kHigh = 2u;
// one table's fences (valid: kLow | kHigh)
struct Fence {
  FKey lo, hi;
  uint32_t valid, pad;
  uint64_t pad2;
};
static_assert(sizeof(Fence) == 80, "Fence is 80 bytes");

// a against b: < 0, 0, > 0
LSMCK_ENC_HD int fkey_cmp(const FKey& a, const FKey& b) {
  if (a.ok.chunk != b.ok.chunk) return a.ok.chunk < b.ok.chunk ? -1 : 1;
  if (a.ok.tail != b.ok.tail) return a.ok.tail < b.ok.tail ? -1 : 1;
  if (a.ok.tail < mem::kMore) return 0;
  return get::bytes_cmp64(a.p + 8u, a.klen - 8u, b.p + 8u, b.klen - 8u);
}
// a fence key against a query
LSMCK_ENC_HD int fkey_cmp(const FKey& a, const get::Key& k) {
  if (a.ok.chunk != k.ok.chunk) return a.ok.chunk < k.ok.chunk ? -1 : 1;
  if (a.ok.tail != k.ok.tail) return a.ok.tail < k.ok.tail ? -1 : 1;
  if (a.ok.tail < mem::kMore) return 0;
  return get::bytes_cmp64(a.p + 8u, a.klen - 8u, k.p + 8u, (uint64_t)k.ok.klen - 8u);
}

// item j of T as a fence key
LSMCK_ENC_HD FKey item_fkey(const get::Table& T, uint64_t j) {
  FKey f;
  f.ok = T.ok[j];
  f.klen = get::item_klen(T.idx, T.ioff[j]);
  f.p = T.idx + T.ioff[j] + 8u;
  return f;
}
// the key of the whole record at pos of T's data image
LSMCK_ENC_HD FKey rec_fkey(const get::Table& T, uint64_t pos, uint32_t klen) {
  const mem::ChunkTail ct = mem::chunk_tail(T.img, pos + sst::kHdr, klen, 0);
  FKey f;
  f.ok.chunk = ct.chunk, f.ok.tail = ct.tail, f.ok.klen = klen;
  f.klen = klen;
  f.p = T.img + pos + sst::kHdr;
  return f;
}

// What scan_range(start, end) visits when nothing matches: at most cap
// records.  floor (optional): false once a visited key lies below it; top
// (optional): raised to the highest visited key.  Returns whether the walk
// ended within the cap.
LSMCK_ENC_HD bool walk(const get::Table& T, uint64_t start, uint64_t end, uint32_t cap, const FKey* floor,
                       bool* above, FKey* top) {
  uint64_t pos = start;
  for (uint32_t seen = 0;; ++seen) {
    uint32_t kl = 0, vl = 0;
    const uint64_t sz = mrg::rec_at(T.img, T.dlen, pos, &kl, &vl);
    if (!sz) return true;
    if (seen == cap) return false;
    const FKey r = rec_fkey(T, pos, kl);
    if (floor && fkey_cmp(r, *floor) < 0) *above = false;
    if (top && fkey_cmp(r, *top) > 0) *top = r;
    pos += sz;
    if (pos >= end) return true;
  }
}

// the fences of T
LSMCK_ENC_HD Fence fences(const get::Table& T, uint32_t cap) {
  Fence F;
  F.valid = 0, F.pad = 0, F.pad2 = 0;
  F.lo.ok.chunk = 0, F.lo.ok.tail = 0, F.lo.ok.klen = 0, F.lo.klen = 0, F.lo.p = nullptr;
  F.hi = F.lo;
  if (!T.nitems) return F;
  F.lo = item_fkey(T, 0);
  bool above = true;
  if (walk(T, 0, T.ipos[0], cap, &F.lo, &above, nullptr) && above) F.valid |= kLow;
  F.hi = item_fkey(T, T.nitems - 1u);
  if (walk(T, T.ipos[T.nitems - 1u], T.dlen, cap, nullptr, nullptr, &F.hi)) F.valid |= kHigh;
  return F;
}

// the literal SsTable::get of k in F's table is None by the fences alone
LSMCK_ENC_HD bool fenced(const Fence& F, const get::Key& k) {
  if ((F.valid & kLow) && fkey_cmp(F.lo, k) > 0) return true;
  return (F.valid & kHigh) && fkey_cmp(F.hi, k) < 0;
}

}  // namespace ts
}  // namespace lsmck
#endif
