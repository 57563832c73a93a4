// lsmck_dbget.h -- the batch Db::get (lsmck_db_get_batch): what the kernels
// (lsmck_dbget.hip dbg_*) and the host model that runs the same code under a
// sanitizer (tests/native/test_dbget.cpp) share.  Internal to liblsmck.so.
//
// Db::get_internal (src/tokio/db.rs:156-189, src/sync/lsm_storage.rs:101): the
// memtable, then the old memtable, then the tables of every level newest
// first; the first Some answers.  Here the memtables are RUNS -- sorted
// arrays of entries over their own arenas, what lsmck_memtable_build leaves --
// and sources 0..nrun-1 are the runs, nrun.. the tables of
// lsmck_sstable_get_batch (lsmck_sstget.h, unchanged).
//   * a run's get is BTreeMap::get (memtable.rs:68-70): the entry whose key is
//     the key, its value whatever it is -- empty, or the one byte 0 that
//     Db::delete inserts (db.rs:140);
//   * Db::get (db.rs:144-155) turns a Some of the one byte 0 into None: the
//     gather gives such a query no byte, as it gives none to a miss.
//
// The device form keeps one order key (mrg::OKey) per run entry; a probe of
// the lower bound reads the two arenas -- the query's and the run's -- only on
// a tie past 8 bytes.  The gather is output-centric as the two encodes' are
// (lsmck_walenc.h): `out` is cut into tiles of enc::kTile bytes aligned on its
// ADDRESS, a lane owns chunks of 16 aligned bytes and writes each with one
// 16-byte store (the arena's first and last partial chunks: byte stores), so
// no byte is written twice and none outside out[0 .. total).
#ifndef LSMCK_DBGET_H
#define LSMCK_DBGET_H
#include <stdint.h>

#include "lsmck.h"
#include "lsmck_sstget.h"

namespace lsmck {
namespace dbg {

static_assert(sizeof(lsmck_get_run) == 48, "lsmck_get_run is 48 bytes");

// ---- the run pass -----------------------------------------------------------

// entry j of run R is one the call takes: the encode's entry rule (type 1,
// 8 + klen + vlen inside u32, non-empty ranges inside the run's own arenas)
LSMCK_ENC_HD bool entry_ok(const lsmck_get_run& R, uint64_t j) {
  return sst::rec_size(R.ents[j], R.keys_bytes, R.vals_bytes) != 0;
}
// its order key
LSMCK_ENC_HD mrg::OKey entry_okey(const lsmck_get_run& R, uint64_t j) { return mrg::okey_of(R.keys, R.ents[j]); }
// entry j >= 1 lies strictly above its predecessor (both taken)
LSMCK_ENC_HD bool entry_above(const lsmck_get_run& R, uint64_t j) {
  const lsmck_wal_cmd a = R.ents[j - 1u], b = R.ents[j];
  return sst::key_less(R.keys + a.key_off, a.klen, R.keys + b.key_off, b.klen);
}
// One thread's work for entry e of all runs (rf: the exclusive scan of the
// runs' nent, nrun + 1): its order key into ok[e]; false when the entry is
// refused (its own rule, or its key is not above its predecessor's).  An
// entry whose predecessor is refused is not compared: that one is reported.
LSMCK_ENC_HD bool run_pass(const lsmck_get_run* runs, const uint64_t* rf, uint64_t nrun, uint64_t e, mrg::OKey* ok) {
  const uint64_t r = mrg::table_of(rf, nrun, e), j = e - rf[r];
  const lsmck_get_run R = runs[r];
  mrg::OKey k;
  k.chunk = 0, k.tail = 0, k.klen = 0;
  const bool good = entry_ok(R, j);
  if (good) k = entry_okey(R, j);
  ok[e] = k;
  if (!good) return false;
  return j == 0 || !entry_ok(R, j - 1u) || entry_above(R, j);
}

// ---- the run probe ----------------------------------------------------------

// a run as the lookups see it: its descriptor and its entries' order keys
struct Run {
  const uint8_t* keys;
  const uint8_t* vals;
  const lsmck_wal_cmd* ents;
  const mrg::OKey* ok;
  uint64_t nent;
};
LSMCK_ENC_HD Run run_of(const lsmck_get_run& R, const mrg::OKey* ok) {
  Run u;
  u.keys = R.keys, u.vals = R.vals, u.ents = R.ents, u.ok = ok, u.nent = R.nent;
  return u;
}

// entry j of R against k: the order keys decide unless both keys go on past 8
// equal bytes; then the two arenas -- the run's and the query's -- from byte 8
LSMCK_ENC_HD int ent_cmp(const Run& R, uint64_t j, const get::Key& k) {
  const mrg::OKey e = R.ok[j];
  if (e.chunk != k.ok.chunk) return e.chunk < k.ok.chunk ? -1 : 1;
  if (e.tail != k.ok.tail) return e.tail < k.ok.tail ? -1 : 1;
  if (e.tail < mem::kMore) return 0;
  return mrg::bytes_cmp(R.keys + R.ents[j].key_off + 8u, e.klen - 8u, k.p + 8u, k.ok.klen - 8u);
}

// BTreeMap::get: the entry of R that holds k (*at), by a lower bound
LSMCK_ENC_HD bool run_get(const Run& R, const get::Key& k, uint64_t* at) {
  uint64_t lo = 0, hi = R.nent;
  bool equal = false;
  while (lo < hi) {
    const uint64_t m = lo + ((hi - lo) >> 1);
    const int c = ent_cmp(R, m, k);
    if (c < 0) {
      lo = m + 1u;
    } else {
      hi = m;
      equal = c == 0;  // (strictly increasing keys: the lower bound is the last m with c >= 0)
    }
  }
  *at = lo;
  return equal;
}

// ---- resolve ----------------------------------------------------------------

// the result of a Some from entry c of run r (val_off: in the run's vals)
LSMCK_ENC_HD lsmck_get_result run_result(const Run& R, const lsmck_wal_cmd& c, uint32_t r) {
  lsmck_get_result x;
  x.val_off = c.vlen ? c.val_off : 0u;  // (an empty value's offset is not looked at)
  if (c.vlen == 1u && R.vals[c.val_off] == 0u) x.val_off |= LSMCK_GET_TOMBSTONE;
  x.vlen = c.vlen;
  x.table = r;
  return x;
}
// Db::get's answer to a result (db.rs:146-151): the bytes the gather owes it
LSMCK_ENC_HD uint64_t answered_len(const lsmck_get_result& x) {
  return x.table == get::kNoTable || (x.val_off & LSMCK_GET_TOMBSTONE) ? 0u : x.vlen;
}

// ---- the gather ---------------------------------------------------------------

constexpr uint32_t kTile = enc::kTile;
constexpr uint32_t kBlock = enc::kBlock;
constexpr int kGroup = enc::kGroup;
// values whose offsets a tile keeps in LDS, in whole loads of the block.  A
// zero-length value starts no byte, so a tile may hold any number of them:
// when more than kSlice values start inside a tile, the tile's chunks search
// off[] itself (Global below) instead of the slice (Slice).
constexpr uint32_t kSlice = 4096u;
constexpr uint32_t kCache = kBlock;  // the tile's first values' source addresses, beside the slice
typedef uint16_t slice_t;
static_assert(kTile <= 32768u && kSlice % kBlock == 0, "slice entries are u16, loaded a block at a time");

struct Tile {
  const uint64_t* off;  // off[0..n]: the exclusive scan of the answered lengths
  const uint64_t* src;  // src[i]: the address of query i's value (not looked at where its length is 0)
  uint64_t n;
  uint64_t r0;    // the value that holds the tile's first byte of out
  int64_t off0;   // its offset
  int64_t ts;     // the tile's start as an offset in out (<= 0 for the first tile)
  int64_t total;  // off[n]
  uint64_t N;     // slice entries, entry 0 (= 0: value r0) included
};

// entry j >= 1 of the tile's slice: value r0 + j's offset less the tile's
// start while it starts inside the tile, kTile (past every chunk) from the
// first one that does not, and past off[n]
LSMCK_ENC_HD uint32_t slice_entry(const uint64_t* off, uint64_t n, uint64_t r0, uint64_t j, int64_t ts) {
  const uint64_t idx = r0 + j;
  if (idx > n) return kTile;
  const int64_t o = (int64_t)off[idx];
  return o < ts + (int64_t)kTile ? (uint32_t)(o - ts) : kTile;
}
// the two forms of the slice: LDS (or a host array), and off[] itself
struct Slice {
  const slice_t* s;
};
struct Global {};
LSMCK_ENC_HD uint32_t rel_at(const Slice& r, const Tile&, uint64_t j) { return r.s[j]; }
LSMCK_ENC_HD uint32_t rel_at(const Global&, const Tile& t, uint64_t j) {
  return j ? slice_entry(t.off, t.n, t.r0, j, t.ts) : 0u;
}

LSMCK_ENC_HD enc::Span span_of(const Tile& t, uint32_t p) {
  enc::Tile e;
  e.ts = t.ts, e.total = t.total;
  return enc::span_of(e, p);
}
// value r0 + j: where it starts in out, and its first byte's address
LSMCK_ENC_HD uint64_t value_src(const Tile& t, const uint64_t* cache, uint64_t j) {
  return j < kCache ? cache[j] : t.src[t.r0 + j];
}
template <class Rel>
LSMCK_ENC_HD int64_t value_start(const Tile& t, Rel rel, uint64_t j) {
  return j ? t.ts + (int64_t)rel_at(rel, t, j) : t.off0;
}

// A chunk in three steps, as enc::chunks takes it (a lane has kGroup chunks'
// source loads in flight):
//   plan():   the chunk's value -- the last j whose offset is at or below the
//             chunk's first byte; among equal offsets that is the one that
//             owns the byte -- and, inside one value, its 16 source bytes;
//   fetch():  enc::fetch;
//   finish(): the funnel and one 16-byte store; or, a chunk that crosses a
//             value's end, byte by byte; partial chunks leave by byte stores.
template <class Rel>
LSMCK_ENC_HD enc::Plan plan(const Tile& t, Rel rel, const uint64_t* cache, uint32_t p) {
  enc::Plan P;
  P.src = nullptr;
  P.j = 0;
  const enc::Span s = span_of(t, p);
  if (s.b0 >= s.b1) return P;
  uint64_t j = 0, z = t.N;
  while (z - j > 1u) {
    const uint64_t m = j + ((z - j) >> 1);
    if (rel_at(rel, t, m) <= p + s.b0) j = m; else z = m;
  }
  P.j = (uint32_t)j;  // (j - 0 < 2^32: n is)
  if (!s.full) return P;
  const uint32_t next = j + 1u < t.N ? rel_at(rel, t, j + 1u) : kTile;
  if (next >= p + 16u) P.src = (const uint8_t*)(uintptr_t)(value_src(t, cache, j) + (uint64_t)(s.pos - value_start(t, rel, j)));
  return P;
}
template <class Rel>
LSMCK_ENC_HD void finish(const Tile& t, Rel rel, const uint64_t* cache, uint32_t p, const enc::Plan& P,
                         const uint32_t (&d)[5], uint8_t* out) {
  const enc::Span s = span_of(t, p);
  if (s.b0 >= s.b1) return;
  uint64_t lo8 = 0, hi8 = 0;
  if (P.src) {
    const uint32_t sh = (uint32_t)((uintptr_t)P.src & 3u);
    lo8 = ((uint64_t)enc::funnel(d[2], d[1], sh) << 32) | enc::funnel(d[1], d[0], sh);
    hi8 = ((uint64_t)enc::funnel(d[4], d[3], sh) << 32) | enc::funnel(d[3], d[2], sh);
  } else {
    uint64_t j = P.j;
    const uint8_t* v = (const uint8_t*)(uintptr_t)value_src(t, cache, j);
    int64_t start = value_start(t, rel, j);
    for (uint32_t b = s.b0; b < s.b1; ++b) {
      bool moved = false;
      while (j + 1u < t.N && rel_at(rel, t, j + 1u) <= p + b) ++j, moved = true;  // (over zero-length values too)
      if (moved) v = (const uint8_t*)(uintptr_t)value_src(t, cache, j), start = value_start(t, rel, j);
      const uint64_t sb = (uint64_t)v[s.pos + b - start] << (8u * (b & 7u));
      if (b & 8u) hi8 |= sb; else lo8 |= sb;
    }
  }
  if (s.full) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 w;
    w.x = (uint32_t)lo8, w.y = (uint32_t)(lo8 >> 32), w.z = (uint32_t)hi8, w.w = (uint32_t)(hi8 >> 32);
    *(u32x4*)(out + s.pos) = w;
#else
    memcpy(out + s.pos, &lo8, 8);
    memcpy(out + s.pos + 8, &hi8, 8);
#endif
  } else {
#pragma clang loop vectorize(disable)  // (byte stores: the vectorizer makes unaligned dword stores of them)
    for (uint32_t b = s.b0; b < s.b1; ++b) out[s.pos + b] = (uint8_t)(((b & 8u) ? hi8 : lo8) >> (8u * (b & 7u)));
  }
}
// the chunks at tile offsets p, p + stride, ... (kGroup of them; those past the tile are skipped)
template <class Rel>
LSMCK_ENC_HD void chunks(const Tile& t, Rel rel, const uint64_t* cache, uint32_t p, uint32_t stride, uint8_t* out) {
  enc::Plan P[kGroup];
  uint32_t d[kGroup][5];
#pragma unroll
  for (int k = 0; k < kGroup; ++k) {
    P[k].src = nullptr, P[k].j = 0;
    if (p + k * stride < kTile) P[k] = plan(t, rel, cache, p + k * stride);
  }
#pragma unroll
  for (int k = 0; k < kGroup; ++k) enc::fetch(P[k], d[k]);
#pragma unroll
  for (int k = 0; k < kGroup; ++k)
    if (p + k * stride < kTile) finish(t, rel, cache, p + k * stride, P[k], d[k], out);
}

}  // namespace dbg
}  // namespace lsmck
#endif
