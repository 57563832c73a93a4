// lsmck_sstmerge.h -- the batch SSTable decode and compaction merge
// (lsmck_sstable_decode_batch, lsmck_sstable_merge_batch): what the kernels
// (lsmck_sstmerge.hip dec_* / mrg_*), the scalar helper
// lsmck_sstable_count_records and the host model that runs the same code under
// a sanitizer (tests/native/test_sstmerge.cpp) share.  Internal to liblsmck.so.
//
// Decode: the batch form of the data file's iterator (src/sync/sstable.rs:77-90
// over datafile.rs:60-83).  From pos = 0 a record is [u32 klen LE][u32 vlen LE]
// [key][val]; UnexpectedEof anywhere -- the header, the key or the value cut --
// ends the table without an error and drops the partial record; pos advances
// by 8 + klen + vlen.  The chain of headers is serial, so the table's index
// file (sstable_index.rs:42-46: u64 count, then u64 klen, key, u64 pos for
// every 100th record) serves as a hint that is proven before it is used: the
// positions cut the table into segments, a thread per segment walks 100
// headers, and the hint stands only when every segment lands on the next
// one's position (the segment walk's induction: segment 0 starts at a record
// by definition, so every landing that checks is a record start).
//
// Merge: the batch form of SsTable::merge_compact's loop
// (src/sync/sstable.rs:171-208).  On strictly increasing tables the loop emits
// every distinct key once, in key order, from the highest-numbered table that
// holds it.  The runs are sorted already, so nothing is sorted again: an entry
// is shadowed when a newer table of its group holds its key (a lower bound
// per newer table), and a live entry's slot is the number of live entries of
// its group with a smaller key (a lower bound per table of the group, into
// the scan of the live flags).  A probe of those searches compares one dense
// 16-byte order key (the key's first 8 bytes big-endian and zero padded, and
// min(klen, 9): mem::chunk_tail) and reads the arena only on a full tie.
#ifndef LSMCK_SSTMERGE_H
#define LSMCK_SSTMERGE_H
#include <stdint.h>
#include <string.h>

#include "lsmck.h"
#include "lsmck_memsort.h"
#include "lsmck_sstenc.h"

namespace lsmck {
namespace mrg {

constexpr uint32_t kStep = sst::kIndexStep;         // records per index item
constexpr uint64_t kMaxTable = 0xFFFFFFFFull;       // a table's data file: under it a record that fits cannot wrap
                                                    // the reference's u32 8 + klen + vlen (datafile.rs:81)

// the 8 bytes at p, little-endian.  On the device from the aligned dwords
// that hold one of them (two or three: no dword without a byte of the range
// is loaded); on the host exactly those bytes, so that a sanitizer sees the
// range itself.
LSMCK_ENC_HD uint64_t load64(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
  const uint8_t* a = p - sh;
  const uint32_t d0 = sst::load32(a), d1 = sst::load32(a + 4), d2 = sh ? sst::load32(a + 8) : 0u;
  return ((uint64_t)enc::funnel(d2, d1, sh) << 32) | enc::funnel(d1, d0, sh);
#else
  uint64_t x;
  memcpy(&x, p, 8);
  return x;
#endif
}

// The iterator's step (datafile.rs:70-83) at pos of an image of len bytes: the
// record's size and its two lengths, or 0 where read_record gives None (fewer
// than 8 bytes left, or the key or the value cut).  len <= kMaxTable.
LSMCK_ENC_HD uint64_t rec_at(const uint8_t* img, uint64_t len, uint64_t pos, uint32_t* klen, uint32_t* vlen) {
  if (pos > len || len - pos < sst::kHdr) return 0;
  const uint64_t h = load64(img + pos);
  *klen = (uint32_t)h;
  *vlen = (uint32_t)(h >> 32);
  const uint64_t sz = (uint64_t)sst::kHdr + *klen + *vlen;
  return sz <= len - pos ? sz : 0;
}

// the record at pos of the table whose image starts at base in the arena, as an entry
LSMCK_ENC_HD lsmck_wal_cmd entry_of(uint64_t base, uint64_t pos, uint32_t klen, uint32_t vlen) {
  lsmck_wal_cmd c;
  c.key_off = base + pos + sst::kHdr;
  c.val_off = c.key_off + klen;
  c.klen = klen;
  c.vlen = vlen;
  c.type = 1u;
  c.reserved = 0u;
  return c;
}

// The whole walk from pos: the records passed (at most `limit`), *end = where
// it stopped; ents (optional) receives them.
LSMCK_ENC_HD uint64_t walk(const uint8_t* img, uint64_t len, uint64_t base, uint64_t pos, uint64_t limit,
                           lsmck_wal_cmd* ents, uint64_t* end) {
  uint64_t c = 0;
  while (c < limit) {
    uint32_t kl = 0, vl = 0;
    const uint64_t sz = rec_at(img, len, pos, &kl, &vl);
    if (!sz) break;
    if (ents) ents[c] = entry_of(base, pos, kl, vl);
    pos += sz;
    ++c;
  }
  *end = pos;
  return c;
}

// a span inside its arena
LSMCK_ENC_HD bool span_ok(uint64_t off, uint64_t len, uint64_t arena) { return off <= arena && len <= arena - off; }

// The index image of one table (sstable_index.rs:42-46, bincode fixint): its
// item count when the image is a usable hint, ~0 when it is not.  Usable: it
// parses to exactly ilen bytes, pos_0 == 0 and the positions increase inside
// dlen.  pos (optional, `cap` entries) receives the positions; an image with
// more items than cap is not usable.
LSMCK_ENC_HD uint64_t index_parse(const uint8_t* idx, uint64_t ilen, uint64_t dlen, uint64_t* pos, uint64_t cap) {
  constexpr uint64_t kNo = ~0ull;
  if (ilen < 8u) return kNo;
  const uint64_t count = load64(idx);
  if (count > (ilen - 8u) / 16u || (pos && count > cap)) return kNo;
  uint64_t q = 8u, prev = 0;
  for (uint64_t j = 0; j < count; ++j) {
    if (ilen - q < 16u) return kNo;
    const uint64_t klen = load64(idx + q);
    if (klen > ilen - q - 16u) return kNo;
    const uint64_t p = load64(idx + q + 8u + klen);
    if (j == 0 ? p != 0 : p <= prev) return kNo;
    if (p >= dlen) return kNo;
    if (pos) pos[j] = p;
    prev = p;
    q += 16u + klen;
  }
  return q == ilen ? count : kNo;
}

// The parse's parallel form, for an index whose keys have one length klen0:
// item j then lies at 8 + j * (16 + klen0).  index_uniform() finds a
// candidate (the count and the first item's klen account for exactly ilen
// bytes); uniform_item() proves item j where it is expected -- its klen is
// klen0 -- and applies the position rules to it.  Item 0 starts at byte 8 by
// definition, and an item at its expected place with that klen puts its
// successor at its expected place: when every item checks, the items are the
// serial parse's.  When one does not, the serial parse decides.
LSMCK_ENC_HD bool index_uniform(const uint8_t* idx, uint64_t ilen, uint64_t* count, uint64_t* klen0) {
  if (ilen < 24u) return false;
  const uint64_t c = load64(idx);
  if (c == 0 || c > (ilen - 8u) / 16u) return false;
  const uint64_t k = load64(idx + 8u);
  if ((ilen - 8u) % c != 0 || (ilen - 8u) / c < 16u || (ilen - 8u) / c - 16u != k) return false;
  *count = c;
  *klen0 = k;
  return true;
}
LSMCK_ENC_HD bool uniform_item(const uint8_t* idx, uint64_t dlen, uint64_t klen0, uint64_t j, uint64_t* pos) {
  const uint8_t* it = idx + 8u + j * (16u + klen0);
  if (load64(it) != klen0) return false;
  const uint64_t p = load64(it + 8u + klen0);
  if (j == 0 ? p != 0 : p <= load64(it - 8u)) return false;  // (it - 8: the item before it ends with its position)
  if (p >= dlen) return false;
  *pos = p;
  return true;
}

// Segment j of a table whose hint has `count` items: the walk from its
// position passes *recs records and stops at *end.  It checks when -- not the
// last -- it passes exactly kStep records and lands on the next item's
// position, or -- the last -- it ends after 1..kStep records where the next
// record no longer fits.
LSMCK_ENC_HD bool seg_check(const uint8_t* img, uint64_t dlen, uint64_t p, bool last, uint64_t next, uint32_t* recs,
                            uint64_t* end) {
  const uint64_t c = walk(img, dlen, 0, p, kStep, nullptr, end);
  *recs = (uint32_t)c;
  if (!last) return c == kStep && *end == next;
  if (c == 0) return false;
  uint32_t kl, vl;
  return c < kStep || rec_at(img, dlen, *end, &kl, &vl) == 0;
}
// an empty table's hint: a count of 0 and no whole record
LSMCK_ENC_HD bool empty_check(const uint8_t* img, uint64_t dlen) {
  uint32_t kl, vl;
  return rec_at(img, dlen, 0, &kl, &vl) == 0;
}

// ---- merge ----------------------------------------------------------------

// an entry's order key: one dense element of the searches
struct OKey {
  uint64_t chunk;  // key bytes [0, 8) big-endian, zero padded
  uint32_t tail;   // min(klen, 9)
  uint32_t klen;
};
LSMCK_ENC_HD OKey okey_of(const uint8_t* keys, const lsmck_wal_cmd& c) {
  const mem::ChunkTail ct = mem::chunk_tail(keys, c.key_off, c.klen, 0);
  OKey k;
  k.chunk = ct.chunk;
  k.tail = ct.tail;
  k.klen = c.klen;
  return k;
}

// the bytes a[0..la) against b[0..lb) in the reference's Vec<u8> order: < 0, 0, > 0
LSMCK_ENC_HD int bytes_cmp(const uint8_t* a, uint32_t la, const uint8_t* b, uint32_t lb) {
  const uint32_t m = la < lb ? la : lb;
  uint32_t i = 0;
  if (m >= 4u && ((((uintptr_t)a) | ((uintptr_t)b)) & 3u) == 0u) {
    for (; i + 4u <= m; i += 4u) {
      const uint32_t x = sst::load32(a + i), y = sst::load32(b + i);
      if (x != y) return __builtin_bswap32(x) < __builtin_bswap32(y) ? -1 : 1;
    }
  }
  for (; i < m; ++i)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return la < lb ? -1 : la > lb ? 1 : 0;
}

// entry (a, its key at keys + a_off) against entry (b, b_off): the order keys
// decide unless both keys go on past 8 equal bytes; then the arena, from byte 8
LSMCK_ENC_HD int okey_cmp(const OKey& a, uint64_t a_off, const OKey& b, uint64_t b_off, const uint8_t* keys) {
  if (a.chunk != b.chunk) return a.chunk < b.chunk ? -1 : 1;
  if (a.tail != b.tail) return a.tail < b.tail ? -1 : 1;
  if (a.tail < mem::kMore) return 0;
  return bytes_cmp(keys + a_off + 8u, a.klen - 8u, keys + b_off + 8u, b.klen - 8u);
}

// the first entry of [lo, hi) whose key is not below k's (hi: none); *equal:
// that entry holds k's key
LSMCK_ENC_HD uint64_t lower_bound(const OKey* ok, const lsmck_wal_cmd* ents, const uint8_t* keys, uint64_t lo,
                                  uint64_t hi, const OKey& k, uint64_t k_off, bool* equal) {
  const uint64_t end = hi;
  while (lo < hi) {
    const uint64_t m = lo + ((hi - lo) >> 1);
    const OKey e = ok[m];
    int c;
    if (e.chunk != k.chunk || e.tail != k.tail || e.tail < mem::kMore)
      c = okey_cmp(e, 0, k, 0, keys);  // (decided without the arena)
    else
      c = okey_cmp(e, ents[m].key_off, k, k_off, keys);
    if (c < 0) lo = m + 1u; else hi = m;
  }
  *equal = false;
  if (lo < end) {
    const OKey e = ok[lo];
    if (e.chunk == k.chunk && e.tail == k.tail)
      *equal = e.tail < mem::kMore || okey_cmp(e, ents[lo].key_off, k, k_off, keys) == 0;
  }
  return lo;
}

// a tombstone: the value is the one byte 0 (sstable.rs:193)
LSMCK_ENC_HD bool tombstone(const lsmck_wal_cmd& c, const uint8_t* vals) { return c.vlen == 1u && vals[c.val_off] == 0u; }

// entry i of table t is shadowed: a newer table of its group, t < s < gend,
// holds its key (the loop's `<=` moves the choice to the later table and the
// earlier table's equal entry is advanced past, sstable.rs:180-185)
LSMCK_ENC_HD bool shadowed(const OKey* ok, const lsmck_wal_cmd* ents, const uint8_t* keys, const uint64_t* tf,
                           uint64_t t, uint64_t gend, uint64_t i) {
  const OKey k = ok[i];
  const uint64_t k_off = ents[i].key_off;
  for (uint64_t s = t + 1u; s < gend; ++s) {
    bool eq;
    (void)lower_bound(ok, ents, keys, tf[s], tf[s + 1u], k, k_off, &eq);
    if (eq) return true;
  }
  return false;
}

// live entry i of table t of the group [gbeg, gend): its place in `out` -- the
// live entries before the group, plus over every table of the group the live
// entries below i's key (lp: the exclusive scan of the live flags; for its own
// table the lower bound is i itself; a key has one live entry at most, so a
// lower bound counts none of its equals)
LSMCK_ENC_HD uint64_t slot_of(const OKey* ok, const lsmck_wal_cmd* ents, const uint8_t* keys, const uint64_t* tf,
                              const uint64_t* lp, uint64_t gbeg, uint64_t gend, uint64_t t, uint64_t i) {
  const OKey k = ok[i];
  const uint64_t k_off = ents[i].key_off;
  uint64_t slot = lp[tf[gbeg]];
  for (uint64_t s = gbeg; s < gend; ++s) {
    bool eq;
    const uint64_t lb = s == t ? i : lower_bound(ok, ents, keys, tf[s], tf[s + 1u], k, k_off, &eq);
    slot += lp[lb] - lp[tf[s]];
  }
  return slot;
}

// the table of entry i: the last t with tf[t] <= i (tf: ntab + 1 values, tf[0] = 0 <= i < tf[ntab])
LSMCK_ENC_HD uint64_t table_of(const uint64_t* tf, uint64_t ntab, uint64_t i) {
  uint64_t lo = 0, hi = ntab;
  while (hi - lo > 1u) {
    const uint64_t m = lo + ((hi - lo) >> 1);
    if (tf[m] <= i) lo = m; else hi = m;
  }
  return lo;
}

}  // namespace mrg
}  // namespace lsmck
#endif
