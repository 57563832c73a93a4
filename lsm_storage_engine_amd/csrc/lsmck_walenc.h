// lsmck_walenc.h -- the batch WAL encode (lsmck_wal_encode_batch): record
// arithmetic and the gather's tile logic, shared by the kernels
// (lsmck_wal.hip wal_encode_*) and the host model that runs the same code
// under a sanitizer (tests/native/test_walenc.cpp).  Internal to liblsmck.so.
//
// The batch form of CommandLog::log (wal.rs:165-196): command i names its key
// in one arena and, for an Insert, its value in another; record i is
//   Insert: [u8 1][u32 crc][u32 klen][u32 vlen][key][val]
//   Remove: [u8 2][u32 crc][u32 klen][key]
// at off[i], the exclusive scan of the record sizes.  The gather is
// output-centric: the image is cut into tiles of kTile bytes aligned on its
// ADDRESS, one per workgroup; a lane owns chunks of 16 aligned bytes and
// writes each with one 16-byte store (the image's first and last partial
// chunks: byte stores of the image's own bytes), so no byte is written twice
// and none outside the image.
#ifndef LSMCK_WALENC_H
#define LSMCK_WALENC_H
#include <stdint.h>
#include <string.h>

#include "lsmck.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LSMCK_ENC_HD __host__ __device__ __forceinline__
#else
#define LSMCK_ENC_HD static inline
#endif

namespace lsmck {
namespace enc {

constexpr uint32_t kTile = 32768u;  // image bytes per workgroup: a power of two, at most 64 KiB
constexpr uint32_t kBlock = 256u;   // threads per workgroup
// records that can start inside a tile behind its first byte: at most
// ceil(kTile / 9) (a record is 9 bytes or more), in whole loads of the block
constexpr uint32_t kSlice = ((kTile + 8u) / 9u + kBlock - 1u) / kBlock * kBlock;
static_assert((kTile & (kTile - 1u)) == 0 && kTile <= 65536u && kTile % (16u * kBlock) == 0, "tile shape");

LSMCK_ENC_HD uint32_t hdr(uint32_t type) { return type == 1u ? 13u : 9u; }
LSMCK_ENC_HD uint32_t vlen_of(const lsmck_wal_cmd& c) { return c.type == 1u ? c.vlen : 0u; }

// the command's record size; 0: invalid (its type, an Insert of more than
// 2^32-1 payload bytes, or a non-empty source range outside its arena)
LSMCK_ENC_HD uint64_t rec_size(const lsmck_wal_cmd& c, uint64_t kb, uint64_t vb) {
  if (c.type != 1u && c.type != 2u) return 0;
  const uint64_t vlen = vlen_of(c);
  if ((uint64_t)c.klen + vlen > 0xFFFFFFFFull) return 0;
  if (c.klen && (c.key_off > kb || c.klen > kb - c.key_off)) return 0;
  if (vlen && (c.val_off > vb || vlen > vb - c.val_off)) return 0;
  return (uint64_t)hdr(c.type) + c.klen + vlen;  // (widened first: klen alone may be 2^32-1)
}

// The tile's first record r0 -- the last one with off[r0] <= t0 -- by a
// search of off[0..n] that probes 64 places per step (one per lane of a wave:
// 4 dependent loads for 2^24 records instead of 24).  Invariant: off[lo] <= t0
// < off[hi].  probe(): lane's index this step, or hi (nothing to load);
// narrow(): the step's outcome from c, the number of lanes whose probe held
// (off[probe] <= t0: monotone, so they are the first c lanes).
LSMCK_ENC_HD uint64_t probe(uint64_t lo, uint64_t hi, uint32_t lane) {
  const uint64_t step = (hi - lo + 63u) >> 6, idx = lo + (lane + 1u) * step;
  return idx < hi ? idx : hi;
}
LSMCK_ENC_HD void narrow(uint64_t& lo, uint64_t& hi, uint32_t c) {
  const uint64_t step = (hi - lo + 63u) >> 6, nhi = lo + ((uint64_t)c + 1u) * step;
  hi = nhi < hi ? nhi : hi;
  lo += (uint64_t)c * step;
}

// entry j >= 1 of the tile's slice: record r0 + j's offset less the tile's
// start ts while the record starts inside the tile, kTile (past every chunk)
// from the first one that does not (and past the last record)
LSMCK_ENC_HD uint32_t slice_entry(const uint64_t* off, uint64_t n, uint64_t r0, uint32_t j, int64_t ts) {
  const uint64_t idx = r0 + j;
  if (idx > n) return kTile;
  const int64_t o = (int64_t)off[idx];
  return o < ts + (int64_t)kTile ? (uint32_t)(o - ts) : kTile;
}

// the commands of the tile's first kCache records are held in LDS beside the
// slice (one coalesced load per tile): a chunk's record then costs no global
// load of its own before the source's
constexpr uint32_t kCache = kBlock;
typedef uint16_t slice_t;  // slice entries: offsets inside a tile, or kTile
static_assert(kTile <= 32768u, "slice entries are u16");
constexpr int kGroup = 4;  // chunks a lane has in flight: their source loads are issued together

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
  uint32_t klen, vlen, type, h;
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
  R.vlen = vlen_of(c);
  R.type = c.type;
  R.h = hdr(c.type);
  return R;
}

// bytes sh..sh+3 of the little-endian pair lo, hi (v_alignbyte)
LSMCK_ENC_HD uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * sh));
#endif
}

// the chunk at tile offset p (a multiple of 16): its image offset and which
// of its bytes [b0, b1) are the image's (none: b0 >= b1)
struct Span {
  int64_t pos;
  uint32_t b0, b1;
  bool full;
};
LSMCK_ENC_HD Span span_of(const Tile& t, uint32_t p) {
  Span s;
  s.pos = t.ts + p;
  s.b0 = s.pos < 0 ? (s.pos + 16 <= 0 ? 16u : (uint32_t)(-s.pos)) : 0u;
  s.b1 = s.pos + 16 <= t.total ? 16u : (s.pos >= t.total ? 0u : (uint32_t)(t.total - s.pos));
  s.full = s.b0 == 0u && s.b1 == 16u;
  return s;
}

// A chunk in three steps, so that a lane takes kGroup chunks through each
// step together and their source loads are in flight at once (one chunk after
// the other, a lane waits out search -> record -> source -> store per chunk).
//   plan():   the chunk's record from the slice by binary search; inside one
//             key or one value it is the fast path, src = its 16 source bytes;
//   fetch():  the fast path's loads: the source's dwords that hold its bytes
//             (four, or five when the source is not dword aligned: every dword
//             loaded holds a byte of the range, so the loads touch only pages
//             that do);
//   finish(): the funnel and one 16-byte store; or, any other chunk (header
//             bytes, a section or record boundary: up to three records of 9
//             bytes), put together byte by byte, the header fields from the
//             command, the CRC field as zeros (wal_encode_stamp writes it);
//             the image's first and last partial chunks leave by byte stores.
struct Plan {
  const uint8_t* src;  // fast path: the chunk's source bytes; else null
  uint32_t j;          // the slice entry of the chunk's first byte
};
template <class Slice, class Cache>
LSMCK_ENC_HD Plan plan(const Tile& t, Slice srel, Cache cache, uint32_t p) {
  Plan P;
  P.src = nullptr;
  P.j = 0;
  const Span s = span_of(t, p);
  if (s.b0 >= s.b1) return P;
  uint32_t j = 0, z = t.N;
  while (z - j > 1u) {  // the last j with srel[j] <= p + b0
    const uint32_t m = (j + z) >> 1;
    if (srel[m] <= p + s.b0) j = m; else z = m;
  }
  P.j = j;
  if (!s.full) return P;
  const Rec R = record(t, srel, cache, j);
  if ((uint64_t)(s.pos - R.start) >= R.h) {
    const uint64_t e = (uint64_t)(s.pos - R.start) - R.h;
    if (e + 16u <= R.klen) P.src = t.keys + R.key_off + e;
    else if (e >= R.klen && e - R.klen + 16u <= R.vlen) P.src = t.vals + R.val_off + (e - R.klen);
  }
  return P;
}
LSMCK_ENC_HD void fetch(const Plan& P, uint32_t (&d)[5]) {
  if (!P.src) return;
  const uint32_t sh = (uint32_t)((uintptr_t)P.src & 3u);
  const uint8_t* a4 = P.src - sh;
#if defined(__HIP_DEVICE_COMPILE__)
  typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));
  const u32x4a4 v = *(const u32x4a4*)a4;
  d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
  d[4] = sh ? *(const uint32_t*)(a4 + 16) : 0u;
#else
  memcpy(d, a4, 16);
  d[4] = 0;
  if (sh) memcpy(d + 4, a4 + 16, 4);
#endif
}
template <class Slice, class Cache>
LSMCK_ENC_HD void finish(const Tile& t, Slice srel, Cache cache, uint32_t p, const Plan& P, const uint32_t (&d)[5],
                         uint8_t* img) {
  const Span s = span_of(t, p);
  if (s.b0 >= s.b1) return;
  uint64_t lo8 = 0, hi8 = 0;
  if (P.src) {
    const uint32_t sh = (uint32_t)((uintptr_t)P.src & 3u);
    lo8 = ((uint64_t)funnel(d[2], d[1], sh) << 32) | funnel(d[1], d[0], sh);
    hi8 = ((uint64_t)funnel(d[4], d[3], sh) << 32) | funnel(d[3], d[2], sh);
  } else {
    uint32_t j = P.j;
    Rec R = record(t, srel, cache, j);
    for (uint32_t b = s.b0; b < s.b1; ++b) {
      while (j + 1u < t.N && srel[j + 1u] <= p + b) R = record(t, srel, cache, ++j);
      const uint64_t q = (uint64_t)(s.pos + b - R.start);
      uint32_t byte;
      if (q < R.h) {
        byte = q == 0 ? R.type
                      : q < 5u ? 0u : q < 9u ? R.klen >> (8u * ((uint32_t)q - 5u)) : R.vlen >> (8u * ((uint32_t)q - 9u));
      } else {
        const uint64_t e = q - R.h;
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
  Plan P[kGroup];
  uint32_t d[kGroup][5];
#pragma unroll
  for (int k = 0; k < kGroup; ++k) {
    P[k].src = nullptr, P[k].j = 0;
    if (p + k * stride < kTile) P[k] = plan(t, srel, cache, p + k * stride);
  }
#pragma unroll
  for (int k = 0; k < kGroup; ++k) fetch(P[k], d[k]);
#pragma unroll
  for (int k = 0; k < kGroup; ++k)
    if (p + k * stride < kTile) finish(t, srel, cache, p + k * stride, P[k], d[k], img);
}

// Record i's payload descriptor for the CRC batch: its payload at off[i] + its
// header.  An empty payload's CRC does not depend on where it is, so it goes
// to its predecessor's payload end -- for a run of up to 8 empty payloads, the
// first one's offset -- as the stream kernel's eligibility rule wants
// (stream_check, lsmck_crc32.hip).  The walk back stops after 8 records: the
// ninth and later ones of a longer run get off[i - 8], which stream_check
// refuses, and the walking kernel takes the batch -- as it would anyway, a
// run of 6 empty records being over the stream kernel's gap limit.
LSMCK_ENC_HD uint64_t payload_desc(const lsmck_wal_cmd* cmds, const uint64_t* off, uint64_t i, uint32_t* len) {
  const lsmck_wal_cmd c = cmds[i];
  *len = c.klen + vlen_of(c);
  if (*len) return off[i] + hdr(c.type);
  uint64_t k = i;
  while (k > 0 && i - k < 8u && cmds[k - 1].klen + vlen_of(cmds[k - 1]) == 0u) --k;
  return off[k];
}

}  // namespace enc
}  // namespace lsmck
#endif
