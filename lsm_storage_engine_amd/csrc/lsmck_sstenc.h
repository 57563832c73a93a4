// lsmck_sstenc.h -- the batch SSTable encode (lsmck_sstable_encode_batch):
// record arithmetic, the key order check and the data gather's tile logic,
// shared by the kernels (lsmck_sstable.hip sst_*) and the host model that runs
// the same code under a sanitizer (tests/native/test_sstenc.cpp).  Internal to
// liblsmck.so.
//
// The batch form of SsTable::from_memtable's file writes (datafile.rs:27-35,
// sstable_index.rs:42-46, checksums.rs:64-80): entry i names its key in one
// arena and its value in another; its record in its table's data file is
//   [u32 klen][u32 vlen][key][val]
// at off[i], the exclusive scan of the record sizes over the whole batch (the
// tables' data files lie back to back, so table boundaries do not exist for
// the gather).  The gather is the WAL encode's (lsmck_walenc.h), with an
// 8-byte header that needs no CRC stamp afterwards: the image is cut into
// tiles of kTile bytes aligned on its ADDRESS, one per workgroup; a lane owns
// chunks of 16 aligned bytes and writes each with one 16-byte store (the
// image's first and last partial chunks: byte stores of the image's own
// bytes), so no byte is written twice and none outside the image.
//
// The tile logic is a copy of lsmck_walenc.h's enc:: functions with the other
// header, not a template over both formats: the WAL kernels keep the code
// they were measured with.  What does not depend on the format is used from
// there (the 64-probe search's probe / narrow, funnel, the fast path's Plan
// and fetch).
//
// One table is one sequential SHA-256 (the digests come from the batch
// SHA-256 dispatcher over the two arenas, a descriptor per table and arena), so
// a single very large table hashes on one lane.
#ifndef LSMCK_SSTENC_H
#define LSMCK_SSTENC_H
#include <stdint.h>
#include <string.h>

#include "lsmck.h"
#include "lsmck_walenc.h"

#ifndef LSMCK_SST_TILE
#define LSMCK_SST_TILE 32768u  // (the host model also builds with 256)
#endif

namespace lsmck {
namespace sst {

constexpr uint32_t kTile = LSMCK_SST_TILE;  // image bytes per workgroup: a power of two, 256 B .. 32 KiB
constexpr uint32_t kBlock = 256u;           // threads per workgroup
constexpr uint32_t kHdr = 8u;               // [u32 klen][u32 vlen]
constexpr uint32_t kMinRec = kHdr;          // an empty key with an empty value
constexpr uint32_t kIndexStep = 100u;       // INDEX_STEP (sstable.rs:17)
// records that can start inside a tile behind its first byte: at most
// ceil(kTile / 8), in whole loads of the block
constexpr uint32_t kSlice = ((kTile + kMinRec - 1u) / kMinRec + kBlock - 1u) / kBlock * kBlock;
static_assert((kTile & (kTile - 1u)) == 0 && kTile >= 256u && kTile <= 32768u, "tile shape (slice entries are u16)");

// the entry's record size; 0: invalid (its type, a record of more than
// 2^32-1 bytes -- the reference forms the size in u32, datafile.rs:34 -- or a
// non-empty source range outside its arena)
LSMCK_ENC_HD uint64_t rec_size(const lsmck_wal_cmd& c, uint64_t kb, uint64_t vb) {
  if (c.type != 1u) return 0;
  if ((uint64_t)kHdr + c.klen + c.vlen > 0xFFFFFFFFull) return 0;
  if (c.klen && (c.key_off > kb || c.klen > kb - c.key_off)) return 0;
  if (c.vlen && (c.val_off > vb || c.vlen > vb - c.val_off)) return 0;
  return (uint64_t)kHdr + c.klen + c.vlen;
}

LSMCK_ENC_HD uint32_t load32(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const uint32_t*)p;
#else
  uint32_t x;
  memcpy(&x, p, 4);
  return x;
#endif
}

// a < b as the reference's BTreeMap<Vec<u8>, _> orders keys: bytewise, the
// shorter one first when it is a prefix.  Dwords where both keys are dword
// aligned (only whole dwords of both keys are loaded), bytes otherwise.
LSMCK_ENC_HD bool key_less(const uint8_t* a, uint32_t la, const uint8_t* b, uint32_t lb) {
  const uint32_t m = la < lb ? la : lb;
  uint32_t i = 0;
  if (m >= 4u && ((((uintptr_t)a) | ((uintptr_t)b)) & 3u) == 0u) {
    for (; i + 4u <= m; i += 4u) {
      const uint32_t x = load32(a + i), y = load32(b + i);
      if (x != y) return __builtin_bswap32(x) < __builtin_bswap32(y);
    }
  }
  for (; i < m; ++i)
    if (a[i] != b[i]) return a[i] < b[i];
  return la < lb;
}

// entries of table's index: every kIndexStep-th one, from its first
LSMCK_ENC_HD uint64_t index_count(uint64_t m) { return (m + kIndexStep - 1u) / kIndexStep; }

// entry j >= 1 of the tile's slice: record r0 + j's offset less the tile's
// start ts while the record starts inside the tile, kTile (past every chunk)
// from the first one that does not (and past the last record)
LSMCK_ENC_HD uint32_t slice_entry(const uint64_t* off, uint64_t n, uint64_t r0, uint32_t j, int64_t ts) {
  const uint64_t idx = r0 + j;
  if (idx > n) return kTile;
  const int64_t o = (int64_t)off[idx];
  return o < ts + (int64_t)kTile ? (uint32_t)(o - ts) : kTile;
}

constexpr uint32_t kCache = kBlock;  // the tile's first records' commands, in LDS beside the slice
typedef uint16_t slice_t;            // slice entries: offsets inside a tile, or kTile
constexpr int kGroup = 4;            // chunks a lane has in flight

struct Tile {
  const uint8_t* keys;
  const uint8_t* vals;
  const lsmck_wal_cmd* cmds;
  uint64_t r0;    // the record that holds the tile's first byte of the image
  int64_t off0;   // its offset
  int64_t ts;     // the tile's start as an image offset (<= 0 for the first tile)
  int64_t total;  // the image's bytes
  uint32_t N;     // slice entries, entry 0 (= 0: record r0) included
};
struct Rec {
  int64_t start;  // the record's header offset in the image
  uint64_t key_off, val_off;
  uint32_t klen, vlen;
};

template <class Slice, class Cache>
LSMCK_ENC_HD Rec record(const Tile& t, Slice srel, Cache cache, uint32_t j) {
  lsmck_wal_cmd c;
  if (j < kCache) c = cache[j]; else c = t.cmds[t.r0 + j];
  Rec R;
  R.start = j ? t.ts + (int64_t)srel[j] : t.off0;
  R.key_off = c.key_off;
  R.val_off = c.val_off;
  R.klen = c.klen;
  R.vlen = c.vlen;
  return R;
}

// byte q < kHdr of the record's header
LSMCK_ENC_HD uint32_t hdr_byte(const Rec& R, uint32_t q) {
  return (q < 4u ? R.klen >> (8u * q) : R.vlen >> (8u * (q - 4u))) & 0xFFu;
}

// the chunk at tile offset p (a multiple of 16): its image offset and which
// of its bytes [b0, b1) are the image's (none: b0 >= b1)
LSMCK_ENC_HD enc::Span span_of(const Tile& t, uint32_t p) {
  enc::Span s;
  s.pos = t.ts + p;
  s.b0 = s.pos < 0 ? (s.pos + 16 <= 0 ? 16u : (uint32_t)(-s.pos)) : 0u;
  s.b1 = s.pos + 16 <= t.total ? 16u : (s.pos >= t.total ? 0u : (uint32_t)(t.total - s.pos));
  s.full = s.b0 == 0u && s.b1 == 16u;
  return s;
}

// A chunk in the WAL gather's three steps (lsmck_walenc.h): plan() finds the
// chunk's record in the slice and, inside one key or one value, its 16 source
// bytes (the fast path); enc::fetch() loads the source's dwords that hold a
// byte of them; finish() funnels them into one 16-byte store, or builds any
// other chunk (header bytes, a section or record boundary: up to three
// records of 8 bytes) byte by byte.
template <class Slice, class Cache>
LSMCK_ENC_HD enc::Plan plan(const Tile& t, Slice srel, Cache cache, uint32_t p) {
  enc::Plan P;
  P.src = nullptr;
  P.j = 0;
  const enc::Span s = span_of(t, p);
  if (s.b0 >= s.b1) return P;
  uint32_t j = 0, z = t.N;
  while (z - j > 1u) {  // the last j with srel[j] <= p + b0
    const uint32_t m = (j + z) >> 1;
    if (srel[m] <= p + s.b0) j = m; else z = m;
  }
  P.j = j;
  if (!s.full) return P;
  const Rec R = record(t, srel, cache, j);
  if ((uint64_t)(s.pos - R.start) >= kHdr) {
    const uint64_t e = (uint64_t)(s.pos - R.start) - kHdr;
    if (e + 16u <= R.klen) P.src = t.keys + R.key_off + e;
    else if (e >= R.klen && e - R.klen + 16u <= R.vlen) P.src = t.vals + R.val_off + (e - R.klen);
  }
  return P;
}
template <class Slice, class Cache>
LSMCK_ENC_HD void finish(const Tile& t, Slice srel, Cache cache, uint32_t p, const enc::Plan& P,
                         const uint32_t (&d)[5], uint8_t* img) {
  const enc::Span s = span_of(t, p);
  if (s.b0 >= s.b1) return;
  uint64_t lo8 = 0, hi8 = 0;
  if (P.src) {
    const uint32_t sh = (uint32_t)((uintptr_t)P.src & 3u);
    lo8 = ((uint64_t)enc::funnel(d[2], d[1], sh) << 32) | enc::funnel(d[1], d[0], sh);
    hi8 = ((uint64_t)enc::funnel(d[4], d[3], sh) << 32) | enc::funnel(d[3], d[2], sh);
  } else {
    uint32_t j = P.j;
    Rec R = record(t, srel, cache, j);
    for (uint32_t b = s.b0; b < s.b1; ++b) {
      while (j + 1u < t.N && srel[j + 1u] <= p + b) R = record(t, srel, cache, ++j);
      const uint64_t q = (uint64_t)(s.pos + b - R.start);
      uint32_t byte;
      if (q < kHdr) {
        byte = hdr_byte(R, (uint32_t)q);
      } else {
        const uint64_t e = q - kHdr;
        byte = e < R.klen ? t.keys[R.key_off + e] : t.vals[R.val_off + (e - R.klen)];
      }
      const uint64_t sb = (uint64_t)(byte & 0xFFu) << (8u * (b & 7u));
      if (b & 8u) hi8 |= sb; else lo8 |= sb;
    }
  }
  if (s.full) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 w;
    w.x = (uint32_t)lo8, w.y = (uint32_t)(lo8 >> 32), w.z = (uint32_t)hi8, w.w = (uint32_t)(hi8 >> 32);
    *(u32x4*)(img + s.pos) = w;
#else
    memcpy(img + s.pos, &lo8, 8);
    memcpy(img + s.pos + 8, &hi8, 8);
#endif
  } else {
#pragma clang loop vectorize(disable)  // (byte stores: the vectorizer makes unaligned dword stores of them)
    for (uint32_t b = s.b0; b < s.b1; ++b) img[s.pos + b] = (uint8_t)(((b & 8u) ? hi8 : lo8) >> (8u * (b & 7u)));
  }
}

// the chunks at tile offsets p, p + stride, ... (kGroup of them; those past the tile are skipped)
template <class Slice, class Cache>
LSMCK_ENC_HD void chunks(const Tile& t, Slice srel, Cache cache, uint32_t p, uint32_t stride, uint8_t* img) {
  enc::Plan P[kGroup];
  uint32_t d[kGroup][5];
#pragma unroll
  for (int k = 0; k < kGroup; ++k) {
    P[k].src = nullptr, P[k].j = 0;
    if (p + k * stride < kTile) P[k] = plan(t, srel, cache, p + k * stride);
  }
#pragma unroll
  for (int k = 0; k < kGroup; ++k) enc::fetch(P[k], d[k]);
#pragma unroll
  for (int k = 0; k < kGroup; ++k)
    if (p + k * stride < kTile) finish(t, srel, cache, p + k * stride, P[k], d[k], img);
}

}  // namespace sst
}  // namespace lsmck
#endif
