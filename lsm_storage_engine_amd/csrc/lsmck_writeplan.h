// lsmck_writeplan.h -- the batch write plan (lsmck_db_write_plan): what the
// kernels (lsmck_writeplan.hip wpl_*), the scalar helper
// (lsmck_db_write_plan_cpu's checks) and the host model that runs the same
// code under a sanitizer (tests/native/test_writeplan.cpp) share.  Internal to
// liblsmck.so.
//
// The batch form of LsmStorage::insert / delete's memtable side
// (src/sync/lsm_storage.rs:59-78, 133-139): commands 0..n-1 go into an empty
// memtable in order, each through MemTable::insert (memtable.rs:72-79) -- a
// delete as the pair (key, [0]) --, and after an Insert, and only then, the
// memtable is flushed when size_in_bytes() >= limit.  With
//   a_i    = klen_i + vlen_i, a delete's vlen being 1
//   prev_i = the last command before i with i's key, or none
// the memtable that starts at command s holds after command i
//   bytes(s, i) = sum over j = s..i of  a_j - [prev_j >= s] * a_{prev_j}
// (an overwrite inside the memtable takes the pair it replaces away), and it
// ends at the first Insert i >= s with bytes(s, i) >= limit.  bytes is not
// monotone in i, so that Insert is found by walking, not by bisection.
//
// The steps, in the kernels' order:
//   prev_of / pack   from the order by (key, log position) that the memtable
//                    build's rounds leave (lsmck_memsort.h): two words a command
//   walk             from every candidate start s, at most `cap` steps: where
//                    the memtable that starts at s ends (kCut), that the log
//                    ends first (kOpen), or that the cap did (kLong)
//   follows          the starts cut into blocks: s's successor lies in s's
//                    block and is known; a block's exits are found by following
//                    these links, the chain of true starts from command 0 hops
//                    from exit to exit and resolves a kLong start by windows
//                    (delta, qualifies)
//   is_entry / entry with every command's segment number: position p of the
//                    order is the last of its (segment, key)
#ifndef LSMCK_WRITEPLAN_H
#define LSMCK_WRITEPLAN_H
#include <stdint.h>

#include "lsmck.h"
#include "lsmck_memsort.h"

namespace lsmck {
namespace wpl {

constexpr uint32_t kNone = 0xFFFFFFFFu;      // prev: no earlier command has the key
constexpr uint64_t kInsertBit = 1ull << 32;  // the packed word: a in bits 0..31, bit 32 = an Insert
// a start's state: what its walk found, and what the chain made of a kLong one
constexpr uint8_t kCut = 0, kOpen = 1, kLong = 2, kLongCut = 3, kLongOpen = 4;

// the value length of the pair a command puts into the memtable: a delete's is [0]
LSMCK_ENC_HD uint32_t ent_vlen(const lsmck_wal_cmd& c) { return c.type == 1u ? c.vlen : 1u; }

// the encode's rule for the entry the command may become (8 + klen + vlen <=
// 2^32-1), which also makes a fit 32 bits
LSMCK_ENC_HD bool fits(const lsmck_wal_cmd& c) { return 8ull + c.klen + ent_vlen(c) <= 0xFFFFFFFFull; }

LSMCK_ENC_HD uint64_t pack(const lsmck_wal_cmd& c) {
  return ((uint64_t)c.klen + ent_vlen(c)) | (c.type == 1u ? kInsertBit : 0ull);
}
LSMCK_ENC_HD uint64_t a_of(uint64_t w) { return w & 0xFFFFFFFFull; }
LSMCK_ENC_HD bool is_insert(uint64_t w) { return (w & kInsertBit) != 0; }

// the tombstone byte a delete's entry points at is missing or not 0
LSMCK_ENC_HD bool tomb_bad(const uint8_t* vals, uint64_t vals_bytes, uint64_t tomb_off) {
  return tomb_off >= vals_bytes || vals[tomb_off] != 0;
}

// perm: the commands by (key, log position); head[p]: position p's key differs
// from position p - 1's.  The command before perm[p] with its key
LSMCK_ENC_HD uint32_t prev_of(const uint32_t* perm, const uint8_t* head, uint64_t p) {
  return (p == 0 || head[p]) ? kNone : perm[p - 1];
}

// command j's share of bytes(s, .): two's complement, the running sum is never negative
LSMCK_ENC_HD uint64_t delta(const uint64_t* aw, const uint32_t* prev, uint64_t s, uint64_t j) {
  uint64_t d = a_of(aw[j]);
  const uint32_t pv = prev[j];
  if (pv != kNone && pv >= s) d -= a_of(aw[pv]);
  return d;
}

// the flush test after command j (lsm_storage.rs:65: >=, and only insert() makes it)
LSMCK_ENC_HD bool qualifies(uint64_t w, uint64_t bytes, uint64_t limit) { return is_insert(w) && bytes >= limit; }

struct Walk {
  uint64_t bytes;  // kCut: size_in_bytes() at the cut; kOpen: at the end of the log
  uint32_t nxt;    // kCut: the next memtable's first command; else n
  uint32_t steps;
  uint8_t state;
};

// the memtable that starts at command s, followed for at most cap commands
LSMCK_ENC_HD Walk walk(const uint64_t* aw, const uint32_t* prev, uint64_t n, uint64_t s, uint64_t limit, uint32_t cap) {
  Walk w;
  w.bytes = 0;
  w.steps = 0;
  uint64_t j = s;
  while (j < n && w.steps < cap) {
    w.bytes += delta(aw, prev, s, j);
    ++w.steps;
    if (qualifies(aw[j], w.bytes, limit)) {
      w.nxt = (uint32_t)(j + 1u);
      w.state = kCut;
      return w;
    }
    ++j;
  }
  w.nxt = (uint32_t)n;
  w.state = j < n ? kLong : kOpen;
  return w;
}

// start s's successor is known from its walk and lies below b1, the end of s's block
LSMCK_ENC_HD bool follows(uint8_t state, uint32_t nxt, uint64_t b1) { return state == kCut && nxt < b1; }

// seg1[c]: command c's segment number plus one.  Position p of the order is
// an entry: the last of its (segment, key) -- inside a run of equal keys the
// log positions increase, so the segments do
LSMCK_ENC_HD bool is_entry(const uint32_t* perm, const uint8_t* head, const uint32_t* seg1, uint64_t n, uint64_t p) {
  if (p + 1u == n || head[p + 1u]) return true;
  return seg1[perm[p + 1u]] != seg1[perm[p]];
}

// the entry of a command: a delete's value is the caller's tombstone byte
LSMCK_ENC_HD lsmck_wal_cmd entry(const lsmck_wal_cmd& c, uint64_t tomb_off) {
  lsmck_wal_cmd e = c;
  if (c.type != 1u) {
    e.val_off = tomb_off;
    e.vlen = 1u;
  }
  e.type = 1u;
  e.reserved = 0u;
  return e;
}

}  // namespace wpl
}  // namespace lsmck
#endif
