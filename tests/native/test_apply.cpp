// The batch command stream's shared logic (csrc/lsmck_apply.h) as a host model:
// every apl:: step in the kernels' order (lsmck_apply.hip) -- the validation,
// the packed words, the two max-scans' inputs and prev / ans / pq from their
// outputs, the forward entry flags, the Gets' and misses' slots and the
// answers -- around the write plan's own steps (lsmck_writeplan.h: the capped
// walks, the blocks' exits, the chain with its windows, the marks, the stable
// sort by segment, the emit with the open segment set first), against the
// literal loop over a std::map: a memtable's map for the writes, and for a Get
// the memtable, then the flushed memtables newest first.  Caps, block sizes
// and window widths from 1 up; the arenas are exact-size heap blocks, so that
// a read past either end is an AddressSanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "lsmck_apply.h"

using namespace lsmck;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_what.c_str()); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)
static std::string g_what;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return g_rng;
}
static uint64_t rnd(uint64_t n) { return rnd() % n; }

struct Stream {
  uint8_t *keys = nullptr, *vals = nullptr;  // exact-size blocks
  uint64_t kb = 0, vb = 0, tomb_off = 0;
  std::vector<lsmck_wal_cmd> cmds;
  ~Stream() {
    free(keys);
    free(vals);
  }
  std::string key(const lsmck_wal_cmd& c) const { return std::string((const char*)keys + c.key_off, c.klen); }
};

// n commands over `distinct` keys of 0..5 bytes, values of 0..vmax bytes (some the one byte 0), one in `del_in` a
// delete, one in `get_in` a Get (0: none)
static void make(Stream& s, size_t n, size_t distinct, uint32_t vmax, unsigned del_in, unsigned get_in,
                 unsigned letters = 2) {
  std::vector<uint32_t> koff(distinct), klen(distinct);
  std::string karena;
  for (size_t d = 0; d < distinct; ++d) {
    koff[d] = (uint32_t)karena.size();
    klen[d] = (uint32_t)rnd(6);
    for (uint32_t j = 0; j < klen[d]; ++j) karena.push_back((char)('a' + rnd(letters)));
  }
  s.kb = karena.size();
  s.keys = (uint8_t*)malloc(s.kb ? s.kb : 1);
  memcpy(s.keys, karena.data(), s.kb);
  s.vb = 64;
  s.vals = (uint8_t*)malloc(s.vb);
  for (uint64_t i = 0; i < s.vb; ++i) s.vals[i] = (uint8_t)(rnd(4) ? 1 + rnd(255) : 0);
  s.tomb_off = s.vb - 1;  // the arena's last byte
  s.vals[s.tomb_off] = 0;
  s.cmds.resize(n);
  for (size_t i = 0; i < n; ++i) {
    lsmck_wal_cmd& c = s.cmds[i];
    const size_t d = rnd(distinct);
    c.key_off = koff[d], c.klen = klen[d];
    c.type = (get_in && rnd(get_in) == 0) ? LSMCK_CMD_GET : rnd(del_in) == 0 ? 2u : 1u;
    c.vlen = (uint32_t)rnd(vmax + 1);
    c.val_off = rnd(s.vb - c.vlen);
    c.reserved = 0xDEAD;
    if (c.type != 1u) c.vlen = 0xFFFFFFFFu, c.val_off = ~0ull;  // not looked at
  }
}

struct Result {
  std::vector<lsmck_write_seg> segs;
  std::vector<lsmck_wal_cmd> ents;
  std::vector<uint32_t> src;
  std::vector<lsmck_apply_get> gets;
  std::vector<lsmck_get_query> miss_q;
  std::vector<uint32_t> miss_get;
  uint64_t nlong = 0;
};

// the literal loop
static Result reference(const Stream& s, uint64_t limit, uint32_t cap) {
  Result r;
  typedef std::map<std::string, std::pair<uint32_t, uint64_t>> Mem;  // key -> (command, klen + vlen)
  Mem mt;
  std::vector<Mem> flushed;
  uint64_t bytes = 0, first = 0;
  auto close = [&](uint64_t next, bool flush) {
    r.segs.push_back({first, (uint64_t)r.ents.size(), bytes});
    if (next - first > cap) ++r.nlong;
    for (const auto& kv : mt) {
      r.ents.push_back(wpl::entry(s.cmds[kv.second.first], s.tomb_off));
      r.src.push_back(kv.second.first);
    }
    if (flush) flushed.push_back(mt);
    mt.clear(), bytes = 0, first = next;
  };
  for (size_t i = 0; i < s.cmds.size(); ++i) {
    const lsmck_wal_cmd& c = s.cmds[i];
    if (c.type == LSMCK_CMD_GET) {
      uint32_t j = apl::kNone, source = LSMCK_GET_NONE;
      auto it = mt.find(s.key(c));
      if (it != mt.end()) {
        j = it->second.first, source = LSMCK_APPLY_MEMTABLE;
      } else {
        for (size_t g = flushed.size(); g-- > 0 && j == apl::kNone;) {
          auto f = flushed[g].find(s.key(c));
          if (f != flushed[g].end()) j = f->second.first, source = (uint32_t)g;
        }
      }
      lsmck_apply_get a;
      a.cmd = (uint32_t)i, a.src_cmd = j, a.source = source, a.val_off = 0, a.vlen = 0;
      if (j != apl::kNone) {
        const lsmck_wal_cmd& w = s.cmds[j];
        if (w.type == 2u) {
          a.val_off = s.tomb_off | LSMCK_GET_TOMBSTONE, a.vlen = 1;
        } else {
          a.vlen = w.vlen, a.val_off = w.vlen ? w.val_off : 0;
          if (w.vlen == 1 && s.vals[w.val_off] == 0) a.val_off |= LSMCK_GET_TOMBSTONE;
        }
      } else {
        r.miss_q.push_back({c.key_off, c.klen, 0});
        r.miss_get.push_back((uint32_t)r.gets.size());
      }
      r.gets.push_back(a);
      continue;
    }
    const uint64_t a = (uint64_t)c.klen + (c.type == 1u ? c.vlen : 1u);
    auto it = mt.find(s.key(c));
    if (it != mt.end()) bytes -= it->second.second;
    mt[s.key(c)] = {(uint32_t)i, a};
    bytes += a;
    if (c.type == 1u && bytes >= limit) close(i + 1, true);
  }
  close(s.cmds.size(), false);
  return r;
}

template <class T>
static void max_scan(const std::vector<T>& in, std::vector<T>& out) {
  T m = 0;
  for (size_t i = 0; i < in.size(); ++i) out[i] = m = std::max(m, in[i]);
}
template <class T>
static void excl_sum(const std::vector<T>& in, std::vector<T>& out) {
  T a = 0;
  for (size_t i = 0; i < in.size(); ++i) out[i] = a, a += in[i];
}

// the kernels' order
static Result model(const Stream& s, uint64_t limit, uint32_t cap, uint32_t B, uint32_t width) {
  const uint64_t n = s.cmds.size();
  const lsmck_wal_cmd* cmds = s.cmds.data();
  Result r;
  // 1. apl_validate
  for (uint64_t i = 0; i < n; ++i) {
    CHECK(apl::valid(cmds[i], s.kb, s.vb) && apl::fits(cmds[i]));
    if (cmds[i].type == 2u) CHECK(!wpl::tomb_bad(s.vals, s.vb, s.tomb_off));
  }
  if (n == 0) {
    r.segs.push_back({0, 0, 0});
    return r;
  }
  // the order (the memtable build's rounds look at key ranges only: here one stable sort)
  std::vector<uint32_t> perm(n);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return s.key(cmds[a]) < s.key(cmds[b]); });
  std::vector<uint8_t> head(n);
  for (uint64_t p = 0; p < n; ++p) head[p] = p != 0 && s.key(cmds[perm[p]]) != s.key(cmds[perm[p - 1]]);  // (head[0] unset)
  // 2. apl_pack, apl_events, the two scans, apl_prev
  std::vector<uint64_t> aw(n);
  std::vector<uint32_t> mark(n, 0), eh(n), ew(n), rs(n), lw(n), prev(n), ans(n), pq(n), act(n + 1), ex(n + 1);
  for (uint64_t c = 0; c < n; ++c) {
    aw[c] = apl::pack(cmds[c]);
    CHECK(apl::word_is_get(aw[c]) == apl::is_get(cmds[c]));
  }
  for (uint64_t p = 0; p < n; ++p) {
    eh[p] = apl::head_word(head.data(), p);
    ew[p] = apl::write_word(!apl::word_is_get(aw[perm[p]]), p);
  }
  max_scan(eh, rs), max_scan(ew, lw);
  for (uint64_t p = 0; p < n; ++p) {
    const uint32_t c = perm[p];
    const bool write = !apl::word_is_get(aw[c]);
    const uint32_t q = apl::prev_pos(rs.data(), lw.data(), p);
    CHECK(q == apl::kNone || (q < p && s.key(cmds[perm[q]]) == s.key(cmds[c]) && !apl::is_get(cmds[perm[q]])));
    const uint32_t pc = q == apl::kNone ? apl::kNone : perm[q];
    prev[c] = write ? pc : apl::kNone, ans[c] = pc, pq[p] = write ? q : apl::kNone, act[p] = write;
  }
  act[n] = 0;
  // the write plan's walks
  std::vector<uint32_t> nxt(n);
  std::vector<uint64_t> byt(n);
  std::vector<uint8_t> state(n);
  uint64_t steps = 0;
  for (uint64_t st = 0; st < n; ++st) {
    const wpl::Walk w = wpl::walk(aw.data(), prev.data(), n, st, limit, cap);
    nxt[st] = w.nxt, byt[st] = w.bytes, state[st] = w.state, steps += w.steps;
  }
  CHECK(steps <= n * (uint64_t)cap);
  // ... the blocks' exits (the links followed one by one), the chain, the marks
  const uint64_t nblk = (n + B - 1) / B;
  auto links = [&](uint64_t b0, uint32_t cnt) {
    std::vector<uint32_t> l(cnt);
    for (uint32_t i = 0; i < cnt; ++i)
      l[i] = wpl::follows(state[b0 + i], nxt[b0 + i], b0 + cnt) ? (uint32_t)(nxt[b0 + i] - b0) : i;
    return l;
  };
  std::vector<uint32_t> exitp(n);
  for (uint64_t b = 0; b < nblk; ++b) {
    const uint64_t b0 = b * B;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(B, n - b0);
    const std::vector<uint32_t> l = links(b0, cnt);
    for (uint32_t i = cnt; i-- > 0;) exitp[b0 + i] = l[i] == i ? (uint32_t)(b0 + i) : exitp[b0 + l[i]];
  }
  std::vector<uint32_t> elist, bfirst(nblk, wpl::kNone);
  bool closed = true;
  for (uint64_t st = 0; st < n;) {
    if (bfirst[st / B] == wpl::kNone) bfirst[st / B] = (uint32_t)elist.size();
    elist.push_back((uint32_t)st);
    const uint32_t e = exitp[st];
    if (state[e] == wpl::kCut) {
      st = nxt[e];
      continue;
    }
    if (state[e] == wpl::kOpen) {
      closed = false;
      break;
    }
    ++r.nlong;
    uint64_t carry = 0, found = ~0ull;
    for (uint64_t base = e; base < n && found == ~0ull; base += width) {
      uint64_t run = carry;
      for (uint64_t j = base; j < std::min<uint64_t>(n, base + width); ++j) {
        run += wpl::delta(aw.data(), prev.data(), e, j);
        if (found == ~0ull && wpl::qualifies(aw[j], run, limit)) {
          found = j;
          byt[e] = run, nxt[e] = (uint32_t)(j + 1), state[e] = wpl::kLongCut;
        }
      }
      carry = run;
    }
    if (found == ~0ull) {
      byt[e] = carry, nxt[e] = (uint32_t)n, state[e] = wpl::kLongOpen;
      closed = false;
      break;
    }
    st = found + 1;
  }
  CHECK(elist.size() <= std::min<uint64_t>(nblk + n / cap + 3, n + 1));
  for (uint64_t b = 0; b < nblk; ++b) {
    if (bfirst[b] == wpl::kNone) continue;
    const uint64_t b0 = b * B;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(B, n - b0);
    const std::vector<uint32_t> l = links(b0, cnt);
    for (size_t k = bfirst[b]; k < elist.size() && elist[k] < b0 + cnt; ++k)
      for (uint32_t i = (uint32_t)(elist[k] - b0);; i = l[i]) {
        CHECK(!mark[b0 + i]);
        mark[b0 + i] = 1;
        if (l[i] == i) break;
      }
  }
  std::vector<uint32_t> seg1(n);
  std::partial_sum(mark.begin(), mark.end(), seg1.begin());
  const uint64_t nseg = seg1[n - 1];
  // 3. apl_clear: one writer a flag
  std::vector<uint8_t> cleared(n, 0);
  for (uint64_t p = 0; p < n; ++p) {
    const uint32_t q = pq[p];
    if (q != apl::kNone && apl::replaces(seg1.data(), perm[p], perm[q])) {
      CHECK(!cleared[q]++);
      act[q] = 0;
    }
  }
  excl_sum(act, ex);
  const uint64_t live = ex[n];
  CHECK(live >= (closed ? nseg : nseg - 1));
  // 4. apl_slots, the two scans and their totals (apl_totals)
  std::vector<uint32_t> gf(n), mf(n), gslot(n), mslot(n);
  for (uint64_t c = 0; c < n; ++c) {
    gf[c] = apl::word_is_get(aw[c]);
    mf[c] = gf[c] && ans[c] == apl::kNone;
  }
  excl_sum(gf, gslot), excl_sum(mf, mslot);
  const uint64_t ngets = (uint64_t)gslot[n - 1] + gf[n - 1], misses = (uint64_t)mslot[n - 1] + mf[n - 1];
  // apl_gets
  r.gets.resize(ngets), r.miss_q.resize(misses), r.miss_get.resize(misses);
  for (uint64_t c = 0; c < n; ++c) {
    if (!apl::is_get(cmds[c])) continue;
    const uint32_t j = ans[c];
    CHECK(gslot[c] < ngets);
    r.gets[gslot[c]] = apl::answer(cmds, s.vals, s.tomb_off, (uint32_t)c, j,
                                   j == apl::kNone ? LSMCK_GET_NONE : apl::source(seg1.data(), (uint32_t)c, j));
    if (j == apl::kNone) {
      CHECK(mslot[c] < misses);
      r.miss_q[mslot[c]] = apl::miss_query(cmds[c]);
      r.miss_get[mslot[c]] = gslot[c];
    }
  }
  // the open segment first (apl_open_seg), then the write plan's compaction, sort by segment, emit and segments
  r.segs.resize(nseg + (closed ? 1 : 0));
  if (!closed) r.segs[nseg - 1] = {0, live, 0};
  std::vector<uint32_t> ekey(live), eval(live);
  for (uint64_t p = 0; p < n; ++p)
    if (act[p]) ekey[ex[p]] = seg1[perm[p]] - 1, eval[ex[p]] = perm[p];
  std::vector<uint32_t> o(live);
  std::iota(o.begin(), o.end(), 0u);
  std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return ekey[a] < ekey[b]; });
  for (size_t j = 0; j < o.size(); ++j) {
    const uint32_t c = eval[o[j]], g = ekey[o[j]];
    r.ents.push_back(wpl::entry(cmds[c], s.tomb_off));
    r.src.push_back(c);
    if (j == 0 || ekey[o[j - 1]] != g) r.segs[g].first_ent = j;
  }
  if (live)
    for (uint64_t c = 0; c < n; ++c)
      if (mark[c]) r.segs[seg1[c] - 1].first_cmd = c, r.segs[seg1[c] - 1].mem_bytes = byt[c];
  if (closed) r.segs[nseg] = {n, live, 0};
  return r;
}

static void compare(const Stream& s, uint64_t limit, uint32_t cap, uint32_t B, uint32_t width) {
  g_what = "n " + std::to_string(s.cmds.size()) + " limit " + std::to_string(limit) + " cap " + std::to_string(cap) +
           " block " + std::to_string(B) + " width " + std::to_string(width);
  const Result want = reference(s, limit, cap), got = model(s, limit, cap, B, width);
  CHECK(got.segs.size() == want.segs.size() && got.ents.size() == want.ents.size());
  for (size_t g = 0; g < want.segs.size(); ++g)
    CHECK(got.segs[g].first_cmd == want.segs[g].first_cmd && got.segs[g].first_ent == want.segs[g].first_ent &&
          got.segs[g].mem_bytes == want.segs[g].mem_bytes);
  CHECK(got.src == want.src);
  CHECK(want.ents.empty() || !memcmp(got.ents.data(), want.ents.data(), want.ents.size() * sizeof(lsmck_wal_cmd)));
  CHECK(got.nlong == want.nlong);
  CHECK(got.gets.size() == want.gets.size() && got.miss_get == want.miss_get);
  for (size_t k = 0; k < want.gets.size(); ++k) {
    const lsmck_apply_get &a = got.gets[k], &b = want.gets[k];
    CHECK(a.val_off == b.val_off && a.vlen == b.vlen && a.source == b.source && a.cmd == b.cmd && a.src_cmd == b.src_cmd);
  }
  for (size_t k = 0; k < want.miss_q.size(); ++k)
    CHECK(got.miss_q[k].key_off == want.miss_q[k].key_off && got.miss_q[k].klen == want.miss_q[k].klen &&
          got.miss_q[k].reserved == 0);
}

int main() {
  static_assert(sizeof(lsmck_apply_get) == 24, "lsmck_apply_get is 24 bytes");
  // the rules by themselves
  {
    lsmck_wal_cmd c{};
    c.type = LSMCK_CMD_GET, c.klen = 0xFFFFFFFFu, c.vlen = 0xFFFFFFFFu, c.val_off = ~0ull;
    CHECK(apl::fits(c) && !apl::valid(c, 100, 0) && apl::pack(c) == 0);  // the entry-length rule is the writes'
    c.klen = 3, c.key_off = 97;
    CHECK(apl::valid(c, 100, 0));
    c.key_off = 98;
    CHECK(!apl::valid(c, 100, 0));
    c.klen = 0, c.key_off = ~0ull;  // an empty key lies anywhere, as for a write
    CHECK(apl::valid(c, 0, 0));
    c.type = 4;
    CHECK(!apl::valid(c, 100, 100));
    c.type = 0;
    CHECK(!apl::valid(c, 100, 100));
    lsmck_wal_cmd e{};
    e.type = 1;  // an Insert of an empty key and value: its word is not a Get's
    CHECK(!apl::word_is_get(apl::pack(e)) && wpl::a_of(apl::pack(e)) == 0);
    const uint8_t head[4] = {0, 0, 1, 0};
    CHECK(apl::head_word(head, 0) == 1 && apl::head_word(head, 1) == 0 && apl::head_word(head, 2) == 3);
    CHECK(apl::write_word(true, 0xFFFFFFFEull) == 0xFFFFFFFFu && apl::write_word(false, 5) == 0);
    const uint32_t rs[4] = {1, 1, 3, 3}, lw[4] = {0, 2, 2, 4};
    CHECK(apl::prev_pos(rs, lw, 0) == apl::kNone && apl::prev_pos(rs, lw, 1) == apl::kNone);
    CHECK(apl::prev_pos(rs, lw, 2) == apl::kNone);  // the last write lies in the run before
    CHECK(apl::prev_pos(rs, lw, 3) == apl::kNone);
    const uint32_t rs2[3] = {1, 1, 1}, lw2[3] = {1, 1, 3};
    CHECK(apl::prev_pos(rs2, lw2, 1) == 0 && apl::prev_pos(rs2, lw2, 2) == 0);
    const uint32_t seg1[3] = {1, 1, 2};
    CHECK(apl::source(seg1, 1, 0) == LSMCK_APPLY_MEMTABLE && apl::source(seg1, 2, 0) == 0 && apl::replaces(seg1, 1, 0));
    CHECK(!apl::replaces(seg1, 2, 1));
  }
  const uint64_t limits[] = {0, 1, 7, 20, 64, 300, ~0ull};
  const uint32_t caps[] = {1, 2, 3, 4, 7, 64, 4096};
  const uint32_t blocks[] = {1, 2, 3, 5, 8, 64, 8192};
  size_t runs = 0;
  for (size_t n : {0, 1, 2, 3, 5, 17, 64, 65, 200, 513}) {
    for (int rep = 0; rep < (n < 100 ? 8 : 3); ++rep) {
      Stream s;
      make(s, n, 1 + rnd(n < 4 ? 3 : n / 2 + 1), rep % 2 ? 12 : 3, rep % 3 == 2 ? 2 : 6, rep % 4 == 3 ? 0 : 2 + rep % 3);
      for (uint64_t limit : limits)
        for (uint32_t cap : caps) {
          const uint32_t B = blocks[rnd(7)], width = (uint32_t)(1 + rnd(9));
          compare(s, limit, cap, B, width);
          ++runs;
        }
      for (uint32_t B : blocks) compare(s, 20, 3, B, 1024), ++runs;
    }
  }
  // only Gets; one key; few keys and mostly Gets
  {
    Stream s;
    make(s, 100, 7, 5, 3, 1);
    for (uint64_t limit : limits) compare(s, limit, 4, 8, 3), ++runs;
    Stream one;
    make(one, 300, 1, 12, 5, 2);
    for (uint64_t limit : limits) compare(one, limit, 4, 8, 3), ++runs;
    Stream few;
    make(few, 400, 3, 12, 4, 1 + 1);
    for (uint64_t limit : limits) compare(few, limit, 64, 64, 1024), ++runs;
  }
  // memtables longer than two of the chain's windows, Gets among their commands
  for (size_t n : {2500, 3100}) {
    Stream s;
    make(s, n, 1200, 12, 6, 3, 26);
    for (uint64_t lim : {(uint64_t)9000, (uint64_t)~0ull})
      for (uint32_t width : {1000u, 1024u})
        for (uint32_t B : {1024u, 1025u, 8192u})
          for (uint32_t cap : {4u, 64u, 4096u}) compare(s, lim, cap, B, width), ++runs;
  }
  printf("apply ok (%zu)\n", runs);
  return 0;
}
