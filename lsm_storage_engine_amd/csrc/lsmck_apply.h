// lsmck_apply.h -- the batch command stream (lsmck_db_apply_plan): what the
// kernels (lsmck_apply.hip apl_*), the scalar helper (lsmck_db_apply_plan_cpu)
// and the host model that runs the same code under a sanitizer
// (tests/native/test_apply.cpp) share.  Internal to liblsmck.so.
//
// The write plan (lsmck_writeplan.h) with Gets between the writes
// (src/command.rs; LsmStorage::get, src/sync/lsm_storage.rs:99-125).  A Get
// changes no memtable: it is a command of a = 0 that is no Insert, so the
// walk, the chain and the marks of the write plan run over the stream as it
// is.  What differs is everything that looks at a key's run in the order by
// (key, log position), where Gets now stand between the writes:
//   prev     a write's predecessor is the last *write* before it in its run,
//            and that write is what answers a Get
//   entry    a write is its (segment, key)'s entry iff no later write of its
//            run has its segment
// Both come from two inclusive max-scans over the positions of the order,
//   rs[p] = max over q <= p of (head[q] ? q + 1 : 0)   the run's start, plus one
//   lw[p] = max over q <= p of (write[q] ? q + 1 : 0)  the last write, plus one
// (position 0 counts as a head): the last write before p is position
// lw[p - 1] - 1, and it lies in p's run iff lw[p - 1] >= rs[p].
#ifndef LSMCK_APPLY_H
#define LSMCK_APPLY_H
#include <stdint.h>

#include "lsmck.h"
#include "lsmck_memsort.h"
#include "lsmck_writeplan.h"

namespace lsmck {
namespace apl {

constexpr uint32_t kNone = wpl::kNone;

LSMCK_ENC_HD bool is_get(const lsmck_wal_cmd& c) { return c.type == LSMCK_CMD_GET; }

// a command the stream takes: a write the memtable build takes, or a Get
// whose key lies inside the key arena (its val_off and vlen are not looked at)
LSMCK_ENC_HD bool valid(const lsmck_wal_cmd& c, uint64_t kb, uint64_t vb) {
  if (!is_get(c)) return mem::valid(c, kb, vb);
  return !(c.klen && (c.key_off > kb || c.klen > kb - c.key_off));
}
// the entry-length rule is the writes'
LSMCK_ENC_HD bool fits(const lsmck_wal_cmd& c) { return is_get(c) || wpl::fits(c); }

// the packed word: a Get adds no bytes and never flushes.  A write's word is
// never 0 but for an Insert of an empty key and an empty value, whose Insert
// bit is set: word == 0 says Get
LSMCK_ENC_HD uint64_t pack(const lsmck_wal_cmd& c) { return is_get(c) ? 0ull : wpl::pack(c); }
LSMCK_ENC_HD bool word_is_get(uint64_t w) { return w == 0; }

// the two scans' inputs at position p
LSMCK_ENC_HD uint32_t head_word(const uint8_t* head, uint64_t p) { return (p == 0 || head[p]) ? (uint32_t)(p + 1u) : 0u; }
LSMCK_ENC_HD uint32_t write_word(bool write, uint64_t p) { return write ? (uint32_t)(p + 1u) : 0u; }

// the position of the last write before p in p's run, or kNone (n < 2^32, so
// every position plus one is a u32 and no position is kNone)
LSMCK_ENC_HD uint32_t prev_pos(const uint32_t* rs, const uint32_t* lw, uint64_t p) {
  if (p == 0) return kNone;
  const uint32_t l = lw[p - 1];
  return (l != 0 && l >= rs[p]) ? l - 1u : kNone;
}

// seg1: a command's segment number plus one.  Write `c`, whose previous write
// of the key is `pc`, takes that one's place as the entry of (segment, key)
LSMCK_ENC_HD bool replaces(const uint32_t* seg1, uint32_t c, uint32_t pc) { return seg1[pc] == seg1[c]; }

// where a Get at command c finds write j's value: its own memtable, or the
// table that j's segment was flushed to
LSMCK_ENC_HD uint32_t source(const uint32_t* seg1, uint32_t c, uint32_t j) {
  return seg1[j] == seg1[c] ? LSMCK_APPLY_MEMTABLE : seg1[j] - 1u;
}

// the Get at command c, answered by write j (kNone: a miss) from `source`;
// vals is read for an Insert of one byte only (Db::get's rule: the byte 0 is a
// tombstone)
LSMCK_ENC_HD lsmck_apply_get answer(const lsmck_wal_cmd* cmds, const uint8_t* vals, uint64_t tomb_off, uint32_t c,
                                    uint32_t j, uint32_t source) {
  lsmck_apply_get g;
  g.cmd = c;
  g.src_cmd = j;
  if (j == kNone) {
    g.val_off = 0, g.vlen = 0, g.source = LSMCK_GET_NONE;
    return g;
  }
  const lsmck_wal_cmd w = cmds[j];
  g.source = source;
  if (w.type != 1u) {
    g.val_off = tomb_off | LSMCK_GET_TOMBSTONE, g.vlen = 1u;
  } else {
    g.vlen = w.vlen;
    g.val_off = w.vlen ? w.val_off : 0ull;
    if (w.vlen == 1u && vals[w.val_off] == 0) g.val_off |= LSMCK_GET_TOMBSTONE;
  }
  return g;
}

// a miss as a query of lsmck_tableset_get_batch / lsmck_db_get_batch over qkeys = keys
LSMCK_ENC_HD lsmck_get_query miss_query(const lsmck_wal_cmd& c) {
  lsmck_get_query q;
  q.key_off = c.key_off, q.klen = c.klen, q.reserved = 0;
  return q;
}

}  // namespace apl
}  // namespace lsmck
#endif
