// lsmck_sstget.h -- the batch point read (lsmck_sstable_get_batch) and its
// scalar form (lsmck_sstable_get): what the kernels (lsmck_sstget.hip get_*),
// the scalar helper in lsmck_cpu.cpp and the host model that runs the same
// code under a sanitizer (tests/native/test_sstget.cpp) share.  Internal to
// liblsmck.so.
//
// SsTable::get (src/sync/sstable.rs:97-113, src/tokio/sstable.rs:57-82),
// literally.  The index file is the bincode fixint image of
// BTreeMap<Vec<u8>, u64> (sstable_index.rs:20-25): u64 count, then u64 klen,
// the key and u64 pos per item.  It is taken as the map when it parses to
// exactly its length and its keys strictly increase in Vec<u8> order -- file
// order is then map order and no key repeats; any other image is refused (the
// reference panics at load, or never writes such a file).  The positions are
// not looked at: they may be any u64 (the decode hint's rules,
// mrg::index_parse, are not the map's).
//   * the map holds the key (sstable.rs:102-106): the value of the record at
//     its position, whatever that record's key is -- the reference does not
//     compare; None where no whole record fits;
//   * otherwise position_range (sstable_index.rs:34-40): start = the position
//     of the last item below the key, or 0; end = that of the first item above
//     it, or data_len; scan_range (datafile.rs:85-103) reads the record at
//     start even when start >= end, returns it when its key is the key, else
//     advances and stops once pos >= end or no whole record fits.
// read_record is mrg::rec_at.  The bloom filter (sstable.rs:98) has no part in
// these calls: a filter built from the table's own keys has no false negatives,
// so it never changes a result, only the work.  An opened table set keeps such
// filters on the device ("bloom_bits", lsmck_bloom.h); the reference's bloom
// file is out of scope here as everywhere in this project.
//
// The device form keeps per item of every table one order key (mrg::OKey), its
// offset in the index arena and its position, so that a probe of the lower
// bound touches the index bytes only on a tie past 8 bytes.
#ifndef LSMCK_SSTGET_H
#define LSMCK_SSTGET_H
#include <stdint.h>

#include "lsmck.h"
#include "lsmck_sstmerge.h"

namespace lsmck {
namespace get {

constexpr uint64_t kNo = ~0ull;
constexpr uint32_t kNoTable = LSMCK_GET_NONE;

// The map's parse: the item count when the image parses to exactly ilen
// bytes, kNo when it does not.  off (optional, `cap` entries) receives the
// items' offsets in the image; an image with more items than cap is kNo.
LSMCK_ENC_HD uint64_t index_parse(const uint8_t* idx, uint64_t ilen, uint64_t* off, uint64_t cap) {
  if (ilen < 8u) return kNo;
  const uint64_t count = mrg::load64(idx);
  if (count > (ilen - 8u) / 16u || (off && count > cap)) return kNo;
  uint64_t q = 8u;
  for (uint64_t j = 0; j < count; ++j) {
    if (ilen - q < 16u) return kNo;
    const uint64_t klen = mrg::load64(idx + q);
    if (klen > ilen - q - 16u) return kNo;
    if (off) off[j] = q;
    q += 16u + klen;
  }
  return q == ilen ? count : kNo;
}

// The parse's parallel form for an index whose keys have one length
// (mrg::index_uniform finds the candidate): item j lies at uniform_off(j) when
// every item before it has that length -- item 0 starts at byte 8 by
// definition, and an item at its expected place with that klen puts its
// successor at its expected place.  When one item does not check, the serial
// parse decides.
LSMCK_ENC_HD uint64_t uniform_off(uint64_t klen0, uint64_t j) { return 8u + j * (16u + klen0); }
LSMCK_ENC_HD bool uniform_item(const uint8_t* idx, uint64_t klen0, uint64_t j) {
  return mrg::load64(idx + uniform_off(klen0, j)) == klen0;
}

// the item at offset `off` of an index image
LSMCK_ENC_HD uint64_t item_klen(const uint8_t* idx, uint64_t off) { return mrg::load64(idx + off); }
LSMCK_ENC_HD uint64_t item_pos(const uint8_t* idx, uint64_t off) {
  return mrg::load64(idx + off + 8u + item_klen(idx, off));
}
// its order key (a length above 2^32-1 is clipped: such a key ties with no query, and lengths are compared below)
LSMCK_ENC_HD mrg::OKey item_okey(const uint8_t* idx, uint64_t off) {
  const uint64_t kl = item_klen(idx, off);
  const uint32_t kl32 = kl > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)kl;
  const mem::ChunkTail ct = mem::chunk_tail(idx, off + 8u, kl32, 0);
  mrg::OKey k;
  k.chunk = ct.chunk, k.tail = ct.tail, k.klen = kl32;
  return k;
}

// a[0..la) against b[0..lb) in Vec<u8> order with 64-bit lengths: < 0, 0, > 0
LSMCK_ENC_HD int bytes_cmp64(const uint8_t* a, uint64_t la, const uint8_t* b, uint64_t lb) {
  uint64_t m = la < lb ? la : lb;
  while (m) {
    const uint32_t step = m > 0x40000000ull ? 0x40000000u : (uint32_t)m;
    const int c = mrg::bytes_cmp(a, step, b, step);
    if (c) return c;
    a += step, b += step, m -= step;
  }
  return la < lb ? -1 : la > lb ? 1 : 0;
}

// the items at offsets a and b of one index image: a's key below b's
LSMCK_ENC_HD bool item_less(const uint8_t* idx, uint64_t a, uint64_t b) {
  const mrg::OKey x = item_okey(idx, a), y = item_okey(idx, b);
  if (x.chunk != y.chunk) return x.chunk < y.chunk;
  if (x.tail != y.tail) return x.tail < y.tail;
  if (x.tail < mem::kMore) return false;  // (equal keys)
  return bytes_cmp64(idx + a + 16u, item_klen(idx, a) - 8u, idx + b + 16u, item_klen(idx, b) - 8u) < 0;
}

// one table as the lookups see it: its data image, its index image and the
// index pass's three values per item
struct Table {
  const uint8_t* img;
  uint64_t dlen;
  const uint8_t* idx;
  const mrg::OKey* ok;
  const uint64_t* ioff;
  const uint64_t* ipos;
  uint64_t nitems;
};
// a query key and its order key
struct Key {
  const uint8_t* p;
  mrg::OKey ok;  // (ok.klen: its length)
};
LSMCK_ENC_HD Key key_of(const uint8_t* qkeys, uint64_t key_off, uint32_t klen) {
  const mem::ChunkTail ct = mem::chunk_tail(qkeys, key_off, klen, 0);
  Key k;
  k.p = klen ? qkeys + key_off : qkeys;  // (an empty key's offset is not looked at)
  k.ok.chunk = ct.chunk, k.ok.tail = ct.tail, k.ok.klen = klen;
  return k;
}
// a query lsmck_sstable_get_batch takes
LSMCK_ENC_HD bool query_ok(const lsmck_get_query& q, uint64_t qb) {
  if (q.reserved != 0u) return false;
  return !q.klen || (q.key_off <= qb && q.klen <= qb - q.key_off);
}

// item j of T against k: the order keys decide unless both keys go on past 8
// equal bytes; then the index bytes, from byte 8
LSMCK_ENC_HD int item_cmp(const Table& T, uint64_t j, const Key& k) {
  const mrg::OKey e = T.ok[j];
  if (e.chunk != k.ok.chunk) return e.chunk < k.ok.chunk ? -1 : 1;
  if (e.tail != k.ok.tail) return e.tail < k.ok.tail ? -1 : 1;
  if (e.tail < mem::kMore) return 0;
  const uint64_t off = T.ioff[j];
  return bytes_cmp64(T.idx + off + 16u, item_klen(T.idx, off) - 8u, k.p + 8u, (uint64_t)k.ok.klen - 8u);
}

// the first item of T whose key is not below k (nitems: none); *equal: it holds k
LSMCK_ENC_HD uint64_t lower_bound(const Table& T, const Key& k, bool* equal) {
  uint64_t lo = 0, hi = T.nitems;
  *equal = false;
  while (lo < hi) {
    const uint64_t m = lo + ((hi - lo) >> 1);
    const int c = item_cmp(T, m, k);
    if (c < 0) {
      lo = m + 1u;
    } else {
      hi = m;
      *equal = c == 0;  // (strictly increasing keys: the lower bound is the last m with c >= 0)
    }
  }
  return lo;
}

// a[8..n) == b[8..n) for keys of n >= 8 bytes whose first 8 bytes are equal:
// 8 bytes a step, the last step over the keys' last 8 bytes
LSMCK_ENC_HD bool rest_equal(const uint8_t* a, const uint8_t* b, uint32_t n) {
  uint32_t i = 8u;
  for (; n - i >= 8u; i += 8u)
    if (mrg::load64(a + i) != mrg::load64(b + i)) return false;
  return i == n || mrg::load64(a + n - 8u) == mrg::load64(b + n - 8u);
}

// scan_range (datafile.rs:85-103).  A step is one round trip: the header and,
// where 16 bytes are left, the 8 bytes behind it -- a key's first 8 -- are
// loaded together; key bytes count only where the length matches, and past
// the first 8 they are read only when those tie.
LSMCK_ENC_HD bool scan_range(const Table& T, const Key& k, uint64_t start, uint64_t end, uint64_t* vpos,
                             uint32_t* vlen) {
  const uint32_t klen = k.ok.klen;
  const uint64_t k0 = __builtin_bswap64(k.ok.chunk);  // (klen >= 8: the key's first 8 bytes as load64 reads them)
  uint64_t pos = start;
  for (;;) {
    uint32_t kl = 0, vl = 0;
    const bool wide = pos <= T.dlen && T.dlen - pos >= 2u * sst::kHdr;
    const uint64_t d0 = wide ? mrg::load64(T.img + pos + sst::kHdr) : 0u;
    const uint64_t sz = mrg::rec_at(T.img, T.dlen, pos, &kl, &vl);
    if (!sz) return false;
    if (kl == klen) {
      const uint8_t* key = T.img + pos + sst::kHdr;
      // (a whole record with a key of 8 bytes or more has 16 bytes left: d0 was loaded)
      const bool eq = klen >= 8u ? d0 == k0 && rest_equal(key, k.p, klen) : mrg::bytes_cmp(key, kl, k.p, kl) == 0;
      if (eq) {
        *vpos = pos + sst::kHdr + kl;
        *vlen = vl;
        return true;
      }
    }
    pos += sz;
    if (pos >= end) return false;
  }
}

// SsTable::get: Some -- the value lies at *vpos of the data image, *vlen
// bytes -- or None.  *walked (optional): the interval was scanned.
LSMCK_ENC_HD bool table_get(const Table& T, const Key& k, uint64_t* vpos, uint32_t* vlen, bool* walked) {
  bool eq;
  const uint64_t lb = lower_bound(T, k, &eq);
  if (walked) *walked = !eq;
  if (eq) {
    uint32_t kl = 0, vl = 0;
    const uint64_t pos = T.ipos[lb];
    if (!mrg::rec_at(T.img, T.dlen, pos, &kl, &vl)) return false;
    *vpos = pos + sst::kHdr + kl;
    *vlen = vl;
    return true;
  }
  const uint64_t start = lb ? T.ipos[lb - 1u] : 0u;
  const uint64_t end = lb < T.nitems ? T.ipos[lb] : T.dlen;
  return scan_range(T, k, start, end, vpos, vlen);
}

// the result of a Some at vpos of the table whose image starts at base in the arena
LSMCK_ENC_HD lsmck_get_result result_of(const uint8_t* img, uint64_t base, uint64_t vpos, uint32_t vlen, uint32_t t) {
  lsmck_get_result r;
  r.val_off = base + vpos;
  if (vlen == 1u && img[vpos] == 0u) r.val_off |= LSMCK_GET_TOMBSTONE;
  r.vlen = vlen;
  r.table = t;
  return r;
}
LSMCK_ENC_HD lsmck_get_result result_none() {
  lsmck_get_result r;
  r.val_off = 0, r.vlen = 0, r.table = kNoTable;
  return r;
}

}  // namespace get
}  // namespace lsmck

#if defined(__HIPCC__)
#include "lsmck_device.h"
namespace lsmck {
namespace get {
// table t and query i of a call's arguments, for the kernels of
// lsmck_sstget.hip and lsmck_dbget.hip
__device__ __forceinline__ Table table_at(const GetArgs& a, uint64_t t) {
  const lsmck_sstable_span s = a.spans[t];
  const uint64_t f = a.itemfirst[t];
  Table T;
  T.img = a.data + s.data_off;
  T.dlen = s.data_len;
  T.idx = a.index + s.index_off;
  T.ok = a.iok + f;
  T.ioff = a.ioff + f;
  T.ipos = a.ipos + f;
  T.nitems = a.itemfirst[t + 1] - f;
  return T;
}
__device__ __forceinline__ Key key_at(const GetArgs& a, uint64_t i) {
  const lsmck_get_query q = a.q[i];
  Key k;
  k.p = q.klen ? a.qkeys + q.key_off : a.qkeys;
  k.ok = a.qok[i];
  return k;
}
}  // namespace get
}  // namespace lsmck
#endif
#endif
