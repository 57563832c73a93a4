// lsmck_bloom.h -- the opened table set's resident bloom filters
// ("bloom_bits"): the hash, the split-block arithmetic and the walks that
// collect a table's key set, which the kernels (lsmck_tableset.hip ts_bloom_*,
// ts_hash, ts_probe<true>) and the host model that runs the same code under a
// sanitizer (tests/native/test_bloom.cpp) share.  Internal to liblsmck.so.
//
// The role of SsTable::get's first line (src/sync/sstable.rs:98: a key the
// filter does not hold is None), not the reference's bloom file: the filter is
// built from the table's own bytes when a set is opened.  For a table with
// index items (key_j, pos_j), j < m, and data length L, its KEY SET is
//   * every item key of at most 2^32-1 bytes (a query's klen is a u32: a
//     longer item key ties with no query), and
//   * the key of every record that ts::walk(T, start_j, end_j, cap) visits,
//     for each interval j = -1 .. m-1: start_-1 = 0, start_j = pos_j, end_j =
//     pos_{j+1} or L behind the last item -- what scan_range visits when
//     nothing matches (the record at start is attempted even when start >=
//     end).  m == 0 has the single walk (0, L).
// A table HAS A FILTER iff each of its m + 1 walks ends within `cap` records
// ("fence_walk_cap") and its block count stays below 2^32.
//
// Exactness.  get::table_get returns Some in two ways only: the query is an
// item key -- it was inserted -- or scan_range(start_{lb-1}, end_{lb-1}) meets
// a record whose key equals the query -- that record is among those walk lb-1
// visits, and it was inserted.  So a query the filter does not hold is None
// under the literal SsTable::get, for positions that are any u64, records
// holding any key, unsorted or cut tails: nothing assumes a well-formed table.
// A table without a filter is simply looked up.
//
// Layout (split-block: a key sets one bit in each of the 8 words of one block).
// nkeys = the item keys taken + the records visited, duplicates counted;
// nblocks = max(1, ceil(nkeys * bits / 256)) blocks of 256 bits, 32-byte
// aligned.  h = mix(klen * 0x9E3779B97F4A7C15), then h = mix(h ^ w) for each
// 8-byte little-endian word w of the key in order, the last one zero-padded
// (mix: splitmix64's finaliser); every key byte and the length enter the hash.
// Block ((h >> 32) * nblocks) >> 32; with x the low 32 bits of h, word i
// carries bit (x * kSalt_i mod 2^32) >> 27.
#ifndef LSMCK_BLOOM_H
#define LSMCK_BLOOM_H
#include <stdint.h>
#include <string.h>

#include "lsmck.h"
#include "lsmck_sstget.h"

namespace lsmck {
namespace blm {

constexpr uint32_t kWords = 8u;  // u32 words of a block
// one table's filter: its first block in the set's filter buffer, its blocks, whether it has one
struct Desc {
  uint64_t first;
  uint32_t nblocks, valid;
};
static_assert(sizeof(Desc) == 16, "Desc is 16 bytes");

LSMCK_ENC_HD uint64_t mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// p[0..r), 1 <= r <= 7, as a little-endian word, zero-padded (the device form
// loads the aligned dwords that hold those bytes, as mrg::load64 does)
LSMCK_ENC_HD uint64_t tail64(const uint8_t* p, uint32_t r) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t sh = (uint32_t)((uintptr_t)p & 3u), n = sh + r;
  const uint8_t* a = p - sh;
  const uint32_t d0 = sst::load32(a), d1 = n > 4u ? sst::load32(a + 4) : 0u, d2 = n > 8u ? sst::load32(a + 8) : 0u;
  const uint64_t w = ((uint64_t)enc::funnel(d2, d1, sh) << 32) | enc::funnel(d1, d0, sh);
  return w & (~0ull >> (64u - 8u * r));
#else
  uint64_t x = 0;
  memcpy(&x, p, r);
  return x;
#endif
}

// the hash of the key p[0..klen)
LSMCK_ENC_HD uint64_t hash(const uint8_t* p, uint64_t klen) {
  uint64_t h = mix(klen * 0x9E3779B97F4A7C15ull);
  uint64_t i = 0;
  for (; klen - i >= 8u; i += 8u) h = mix(h ^ mrg::load64(p + i));
  if (i < klen) h = mix(h ^ tail64(p + i, (uint32_t)(klen - i)));
  return h;
}

LSMCK_ENC_HD uint32_t block_of(uint64_t h, uint32_t nblocks) { return (uint32_t)(((h >> 32) * nblocks) >> 32); }
LSMCK_ENC_HD uint32_t bit_of(uint32_t x, uint32_t salt) { return 1u << ((x * salt) >> 27); }
struct Mask {
  uint32_t w[kWords];
};
LSMCK_ENC_HD Mask mask_of(uint64_t h) {
  const uint32_t x = (uint32_t)h;
  Mask m;
  m.w[0] = bit_of(x, 0x47b6137bu), m.w[1] = bit_of(x, 0x44974d91u), m.w[2] = bit_of(x, 0x8824ad5bu);
  m.w[3] = bit_of(x, 0xa2b7289du), m.w[4] = bit_of(x, 0x705495c7u), m.w[5] = bit_of(x, 0x2df1424bu);
  m.w[6] = bit_of(x, 0x9efc4947u), m.w[7] = bit_of(x, 0x5c6bfb31u);
  return m;
}

// The blocks of nkeys keys at `bits` per key (exact: nkeys = 256 a + b gives a
// bits + ceil(b bits / 256)), or 0 where they would reach 2^32: no filter.
LSMCK_ENC_HD uint32_t nblocks_of(uint64_t nkeys, uint32_t bits) {
  const uint64_t a = nkeys >> 8, b = nkeys & 255u;
  if (a >= (1ull << 32)) return 0;
  const uint64_t nb = a * bits + ((b * bits + 255u) >> 8);
  return nb >= (1ull << 32) ? 0u : nb ? (uint32_t)nb : 1u;
}

// ORs h's eight bits into its block (the device form: 32-bit atomics whose result is not used)
LSMCK_ENC_HD void insert(uint32_t* filt, const Desc& d, uint64_t h) {
  uint32_t* b = filt + (d.first + block_of(h, d.nblocks)) * kWords;
  const Mask m = mask_of(h);
  for (uint32_t i = 0; i < kWords; ++i) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_or(b + i, m.w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    b[i] |= m.w[i];
#endif
  }
}
// all eight bits of h are set in the block's words
LSMCK_ENC_HD bool holds(const uint32_t* block, uint64_t h) {
  const Mask m = mask_of(h);
  uint32_t miss = 0;
  for (uint32_t i = 0; i < kWords; ++i) miss |= ~block[i] & m.w[i];
  return miss == 0;
}
LSMCK_ENC_HD const uint32_t* block_at(const uint32_t* filt, const Desc& d, uint64_t h) {
  return filt + (d.first + block_of(h, d.nblocks)) * kWords;
}

// interval j of T, 0 <= j <= m (interval j - 1 of the definition above)
LSMCK_ENC_HD void interval(const get::Table& T, uint64_t j, uint64_t* start, uint64_t* end) {
  *start = j ? T.ipos[j - 1u] : 0u;
  *end = j < T.nitems ? T.ipos[j] : T.dlen;
}
// interval j has an item key that is taken: item j - 1, where its length is a query's
LSMCK_ENC_HD bool item_taken(const get::Table& T, uint64_t j) {
  return j && get::item_klen(T.idx, T.ioff[j - 1u]) <= 0xFFFFFFFFull;
}

// ts::walk(T, start, end, cap) with f(key, klen) for every visited record.
// *n: the records visited.  Returns whether the walk ended within the cap.
template <typename F>
LSMCK_ENC_HD bool walk_keys(const get::Table& T, uint64_t start, uint64_t end, uint32_t cap, uint64_t* n, F&& f) {
  uint64_t pos = start;
  for (uint32_t seen = 0;; ++seen) {
    uint32_t kl = 0, vl = 0;
    const uint64_t sz = mrg::rec_at(T.img, T.dlen, pos, &kl, &vl);
    *n = seen;
    if (!sz) return true;
    if (seen == cap) return false;
    f(T.img + pos + sst::kHdr, kl);
    *n = seen + 1u;
    pos += sz;
    if (pos >= end) return true;
  }
}

// pass 1, interval j of T: *n = its keys (the item key taken and the records visited); false: the walk passed the cap
LSMCK_ENC_HD bool count(const get::Table& T, uint64_t j, uint32_t cap, uint64_t* n) {
  uint64_t start, end;
  interval(T, j, &start, &end);
  const bool ok = walk_keys(T, start, end, cap, n, [](const uint8_t*, uint32_t) {});
  if (item_taken(T, j)) ++*n;
  return ok;
}
// pass 2, interval j of T, a table with a filter: the same keys into d's blocks
LSMCK_ENC_HD void fill(const get::Table& T, uint64_t j, uint32_t cap, uint32_t* filt, const Desc& d) {
  uint64_t start, end, n;
  interval(T, j, &start, &end);
  (void)walk_keys(T, start, end, cap, &n, [&](const uint8_t* k, uint32_t kl) { insert(filt, d, hash(k, kl)); });
  if (item_taken(T, j)) {
    const uint64_t off = T.ioff[j - 1u];
    insert(filt, d, hash(T.idx + off + 8u, get::item_klen(T.idx, off)));
  }
}

// Interval <-> table: the set's intervals are numbered table by table, table
// t's m_t + 1 from itemfirst[t] + t on (itemfirst: the exclusive scan of the
// m_t, ntab + 1 entries).  The table of interval g < itemfirst[ntab] + ntab.
LSMCK_ENC_HD uint64_t interval_first(const uint64_t* itemfirst, uint64_t t) { return itemfirst[t] + t; }
LSMCK_ENC_HD uint64_t interval_table(const uint64_t* itemfirst, uint64_t ntab, uint64_t g) {
  uint64_t lo = 0, hi = ntab;
  while (hi - lo > 1u) {
    const uint64_t m = lo + ((hi - lo) >> 1);
    if (interval_first(itemfirst, m) <= g) lo = m; else hi = m;
  }
  return lo;
}

// the filter drops the pair (a query of hash h, the table of d): its get is None
LSMCK_ENC_HD bool drops(const uint32_t* filt, const Desc& d, uint64_t h) {
  return d.valid && !holds(block_at(filt, d, h), h);
}

}  // namespace blm
}  // namespace lsmck
#endif
