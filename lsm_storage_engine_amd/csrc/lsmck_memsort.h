// lsmck_memsort.h -- the batch memtable build (lsmck_memtable_build): what the
// kernels (lsmck_memtable.hip mem_*) and the host model that runs the same
// code under a sanitizer (tests/native/test_memsort.cpp) share.  Internal to
// liblsmck.so.
//
// The batch form of MemTable::from_log's map (src/memtable.rs:28-47): the
// commands of a log, in log order, become the live entries in the BTreeMap's
// key order -- bytewise, unsigned, a proper prefix first (sst::key_less) -- the
// last writer of a key winning, a key whose last command is a Remove gone.
//
// Keys are byte strings of any length, so the order is refined 8 key bytes a
// round.  perm[0..n) holds the commands in the order found so far; a GROUP is
// a contiguous range of perm whose keys are equal in their first 8r bytes and
// all go on past them.  Round r forms for every element of a group still
// active
//   chunk = key bytes [8r, 8r + 8) as a big-endian u64, zero padded
//   tail  = min(klen - 8r, 9): 0..8 = the key ends in this chunk with that
//           many bytes, 9 = it goes on
// and sorts the active elements stably by (group, chunk, tail).  Inside a group
// that is the reference's order: the padding is 0, so a key that ended ties
// with or sorts below one with a real byte there, and tail puts the shorter
// one first.  The runs of equal (group, chunk, tail) are the new groups: a run
// with tail <= 8 is one key repeated and is finished, a run of one is
// finished, a run of two or more with tail == 9 stays active.  Every sort pass
// is stable, so equal keys keep their log order and the last of a run of equal
// keys is the key's last writer.
#ifndef LSMCK_MEMSORT_H
#define LSMCK_MEMSORT_H
#include <stdint.h>
#include <string.h>

#include "lsmck.h"
#include "lsmck_sstenc.h"

namespace lsmck {
namespace mem {

constexpr uint32_t kMore = 9u;  // tail: the key goes on past this chunk

// a command the build takes: an Insert or a Remove whose non-empty key, and
// for an Insert whose non-empty value, lies inside its arena (a Remove's
// val_off and vlen are not looked at)
LSMCK_ENC_HD bool valid(const lsmck_wal_cmd& c, uint64_t kb, uint64_t vb) {
  if (c.type != 1u && c.type != 2u) return false;
  if (c.klen && (c.key_off > kb || c.klen > kb - c.key_off)) return false;
  if (c.type == 1u && c.vlen && (c.val_off > vb || c.vlen > vb - c.val_off)) return false;
  return true;
}

struct ChunkTail {
  uint64_t chunk;
  uint32_t tail;
};

// round r's (chunk, tail) of the key keys[key_off .. key_off + klen).  The
// chunk's 1..8 bytes come from the aligned dwords that hold at least one of
// them (up to three), funnelled and byte-swapped: no dword without a byte of
// the key is loaded, so a key may lie at the first and at the last byte of an
// arena whose aligned dwords are readable (enc::fetch's contract).
LSMCK_ENC_HD ChunkTail chunk_tail(const uint8_t* keys, uint64_t key_off, uint32_t klen, uint64_t r) {
  ChunkTail o;
  o.chunk = 0;
  const uint64_t at = 8u * r;
  if (at >= klen) {  // (round 0's empty key; no later round sees an ended key)
    o.tail = 0;
    return o;
  }
  const uint64_t left = klen - at;
  o.tail = left > 8u ? kMore : (uint32_t)left;
  const uint32_t nb = left > 8u ? 8u : (uint32_t)left;  // 1..8 bytes
  const uint8_t* p = keys + key_off + at;
  const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
  const uint8_t* a = p - sh;
  const uint32_t last = (sh + nb - 1u) >> 2;  // the last dword with a byte of the chunk: 0..2
  const uint32_t d0 = sst::load32(a);
  const uint32_t d1 = last >= 1u ? sst::load32(a + 4) : 0u;
  const uint32_t d2 = last >= 2u ? sst::load32(a + 8) : 0u;
  uint64_t v = ((uint64_t)enc::funnel(d2, d1, sh) << 32) | enc::funnel(d1, d0, sh);
  if (nb < 8u) v &= (1ull << (8u * nb)) - 1u;
  o.chunk = __builtin_bswap64(v);  // the key's first byte is the most significant
  return o;
}

// the regroup predicate: two neighbours of the sorted active elements lie in
// one run
LSMCK_ENC_HD bool same_run(uint32_t ga, uint64_t ca, uint32_t ta, uint32_t gb, uint64_t cb, uint32_t tb) {
  return ga == gb && ca == cb && ta == tb;
}
// an element of a run of `more than one` with this tail is refined further
LSMCK_ENC_HD bool stays_active(uint32_t tail, bool run_of_two_or_more) { return tail == kMore && run_of_two_or_more; }

// Position p's share of the reference's size_in_bytes() after from_log
// (memtable.rs:37-45), the commands in (key, log position) order in perm and
// head[p] != 0 where position p's key differs from position p - 1's: an Insert
// adds klen + vlen, also one that overwrites; a Remove whose predecessor has
// its key and is an Insert takes that Insert's klen + vlen away.
LSMCK_ENC_HD int64_t contribution(const lsmck_wal_cmd* cmds, const uint32_t* perm, const uint8_t* head, uint64_t p) {
  const lsmck_wal_cmd c = cmds[perm[p]];
  if (c.type == 1u) return (int64_t)((uint64_t)c.klen + c.vlen);
  if (p == 0 || head[p]) return 0;
  const lsmck_wal_cmd q = cmds[perm[p - 1]];
  return q.type == 1u ? -(int64_t)((uint64_t)q.klen + q.vlen) : 0;
}

// position p holds its key's last writer, and that is an Insert: a live entry
LSMCK_ENC_HD bool live(const lsmck_wal_cmd* cmds, const uint32_t* perm, const uint8_t* head, uint64_t n, uint64_t p) {
  return (p + 1u == n || head[p + 1u]) && cmds[perm[p]].type == 1u;
}

// The replay's compact record as a command over the log image (keys == vals ==
// the image): what the reference's iterator hands to from_log (wal.rs:129-142).
// The payload read is the u32 sum klen + vlen, short at the end of the log; an
// Insert's value is what follows the key in it, a Remove's key all of it.  An
// Insert whose key is longer than the payload read is where split_off panics:
// its key is left reaching past the image (or, for a wrapped sum inside a log
// above 4 GiB, moved there), so that mem::valid refuses it.
LSMCK_ENC_HD lsmck_wal_cmd rec_to_cmd(const lsmck_wal_rec16& r, uint64_t img_bytes) {
  lsmck_wal_cmd c;
  const bool rem = (r.payload_type & LSMCK_WAL_REC16_REMOVE) != 0;
  c.key_off = r.payload_type & LSMCK_WAL_REC16_OFF_MASK;
  c.klen = r.klen;
  c.vlen = rem ? 0u : r.vlen;
  c.type = rem ? 2u : 1u;
  c.reserved = 0;
  const uint64_t avail = c.key_off < img_bytes ? img_bytes - c.key_off : 0;
  uint64_t dlen = (uint32_t)(c.klen + c.vlen);  // (u32: wal.rs:129)
  if (dlen > avail) dlen = avail;
  if (rem) {
    c.klen = (uint32_t)dlen;
  } else if (c.klen > dlen) {
    if ((uint64_t)c.klen <= avail) c.key_off = img_bytes;  // (klen > 0 here)
  } else {
    c.vlen = (uint32_t)(dlen - c.klen);
  }
  c.val_off = c.key_off + c.klen;
  return c;
}

}  // namespace mem
}  // namespace lsmck
#endif
