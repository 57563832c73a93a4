// The batch write plan's shared logic (csrc/lsmck_writeplan.h) as a host model:
// every wpl:: step in the kernels' order (lsmck_writeplan.hip) -- prev and the
// packed words from the order, the capped walks, the blocks' exits by pointer
// doubling, the chain with its windows for a LONG start, the marks, the
// segment numbers, the entries and the stable sort by segment -- with
// std::stable_sort in place of the device's sorts, against the literal loop of
// LsmStorage::insert / delete over a std::map.  Caps, block sizes and window
// widths from 1 up; the arenas are exact-size heap blocks, so that a read past
// either end is an AddressSanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "lsmck_options.h"
#include "lsmck_writeplan.h"

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

// n commands over `distinct` keys of 0..5 bytes from `letters` letters, values of 0..vmax bytes, one in `del_in` a
// delete
static void make(Stream& s, size_t n, size_t distinct, uint32_t vmax, unsigned del_in, unsigned letters = 2) {
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
  for (uint64_t i = 0; i < s.vb; ++i) s.vals[i] = (uint8_t)(1 + rnd(255));
  s.tomb_off = s.vb - 1;  // the arena's last byte
  s.vals[s.tomb_off] = 0;
  s.cmds.resize(n);
  for (size_t i = 0; i < n; ++i) {
    lsmck_wal_cmd& c = s.cmds[i];
    const size_t d = rnd(distinct);
    c.key_off = koff[d], c.klen = klen[d];
    c.type = rnd(del_in) == 0 ? 2u : 1u;
    c.vlen = (uint32_t)rnd(vmax + 1);
    c.val_off = rnd(s.vb - c.vlen);
    c.reserved = 0xDEAD;
    if (c.type == 2u) c.vlen = 0xFFFFFFFFu, c.val_off = ~0ull;  // not looked at
  }
}

struct Result {
  std::vector<lsmck_write_seg> segs;
  std::vector<lsmck_wal_cmd> ents;
  std::vector<uint32_t> src;
  uint64_t nlong = 0;
};

// the literal loop
static Result reference(const Stream& s, uint64_t limit, uint32_t cap) {
  Result r;
  std::map<std::string, std::pair<uint32_t, uint64_t>> mt;  // key -> (command, klen + vlen)
  uint64_t bytes = 0, first = 0;
  auto close = [&](uint64_t next) {
    r.segs.push_back({first, (uint64_t)r.ents.size(), bytes});
    if (next - first > cap) ++r.nlong;
    for (const auto& kv : mt) {
      r.ents.push_back(wpl::entry(s.cmds[kv.second.first], s.tomb_off));
      r.src.push_back(kv.second.first);
    }
    mt.clear(), bytes = 0, first = next;
  };
  for (size_t i = 0; i < s.cmds.size(); ++i) {
    const lsmck_wal_cmd& c = s.cmds[i];
    const uint64_t a = (uint64_t)c.klen + (c.type == 1u ? c.vlen : 1u);
    auto it = mt.find(s.key(c));
    if (it != mt.end()) bytes -= it->second.second;
    mt[s.key(c)] = {(uint32_t)i, a};
    bytes += a;
    if (c.type == 1u && bytes >= limit) close(i + 1);
  }
  close(s.cmds.size());
  return r;
}

// the kernels' order
static Result model(const Stream& s, uint64_t limit, uint32_t cap, uint32_t B, uint32_t width) {
  const uint64_t n = s.cmds.size();
  const lsmck_wal_cmd* cmds = s.cmds.data();
  Result r;
  for (uint64_t i = 0; i < n; ++i) {
    CHECK(mem::valid(cmds[i], s.kb, s.vb) && wpl::fits(cmds[i]));
    if (cmds[i].type == 2u) CHECK(!wpl::tomb_bad(s.vals, s.vb, s.tomb_off));
  }
  if (n == 0) {
    r.segs.push_back({0, 0, 0});
    return r;
  }
  // 1. the order (the memtable build's rounds, here one stable sort), prev, the packed words
  std::vector<uint32_t> perm(n);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return s.key(cmds[a]) < s.key(cmds[b]); });
  std::vector<uint8_t> head(n);
  for (uint64_t p = 0; p < n; ++p) head[p] = p == 0 || s.key(cmds[perm[p]]) != s.key(cmds[perm[p - 1]]);
  std::vector<uint32_t> prev(n);
  std::vector<uint64_t> aw(n);
  for (uint64_t p = 0; p < n; ++p) {
    prev[perm[p]] = wpl::prev_of(perm.data(), head.data(), p);
    aw[p] = wpl::pack(cmds[p]);
  }
  // 2. the walks
  std::vector<uint32_t> nxt(n);
  std::vector<uint64_t> byt(n);
  std::vector<uint8_t> state(n);
  uint64_t steps = 0;
  for (uint64_t st = 0; st < n; ++st) {
    const wpl::Walk w = wpl::walk(aw.data(), prev.data(), n, st, limit, cap);
    nxt[st] = w.nxt, byt[st] = w.bytes, state[st] = w.state, steps += w.steps;
    CHECK(w.steps <= cap && (w.state != wpl::kCut || (w.nxt > st && w.nxt <= n)));
  }
  CHECK(steps <= n * (uint64_t)cap);
  // 3. the blocks' exits by pointer doubling
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
    std::vector<uint32_t> l = links(b0, cnt), t(cnt);
    for (unsigned round = 0;; ++round) {
      bool changed = false;
      for (uint32_t i = 0; i < cnt; ++i) t[i] = l[l[i]], changed |= t[i] != l[i];
      l = t;
      if (!changed) break;
      CHECK(round <= 32);
    }
    for (uint32_t i = 0; i < cnt; ++i) exitp[b0 + i] = (uint32_t)(b0 + l[i]);
  }
  // ... the chain
  std::vector<uint32_t> elist, bfirst(nblk, wpl::kNone);
  bool closed = true;
  for (uint64_t st = 0; st < n;) {
    if (bfirst[st / B] == wpl::kNone) bfirst[st / B] = (uint32_t)elist.size();
    elist.push_back((uint32_t)st);
    const uint32_t e = exitp[st];
    if (state[e] == wpl::kCut) {
      CHECK(nxt[e] >= (e / B + 1) * (uint64_t)B || nxt[e] == n);
      st = nxt[e];
      continue;
    }
    if (state[e] == wpl::kOpen) {
      closed = false;
      break;
    }
    CHECK(state[e] == wpl::kLong);
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
  CHECK(std::is_sorted(elist.begin(), elist.end()));
  // ... the marks
  std::vector<uint32_t> mark(n, 0), seg1(n);
  for (uint64_t b = 0; b < nblk; ++b) {
    if (bfirst[b] == wpl::kNone) continue;
    const uint64_t b0 = b * B;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(B, n - b0);
    const std::vector<uint32_t> l = links(b0, cnt);
    for (size_t k = bfirst[b]; k < elist.size() && elist[k] < b0 + cnt; ++k) {
      CHECK(elist[k] >= b0);
      for (uint32_t i = (uint32_t)(elist[k] - b0);; i = l[i]) {
        CHECK(!mark[b0 + i]);
        mark[b0 + i] = 1;
        if (l[i] == i) break;
      }
    }
  }
  // 4. the segment numbers, the entries, the stable sort by segment
  std::partial_sum(mark.begin(), mark.end(), seg1.begin());
  const uint64_t nseg = seg1[n - 1];
  std::vector<uint32_t> ekey, eval;
  for (uint64_t p = 0; p < n; ++p)
    if (wpl::is_entry(perm.data(), head.data(), seg1.data(), n, p))
      ekey.push_back(seg1[perm[p]] - 1), eval.push_back(perm[p]);
  std::vector<uint32_t> o(ekey.size());
  std::iota(o.begin(), o.end(), 0u);
  std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return ekey[a] < ekey[b]; });
  r.segs.resize(nseg + (closed ? 1 : 0));
  for (size_t j = 0; j < o.size(); ++j) {
    const uint32_t c = eval[o[j]], g = ekey[o[j]];
    r.ents.push_back(wpl::entry(cmds[c], s.tomb_off));
    r.src.push_back(c);
    if (j == 0 || ekey[o[j - 1]] != g) r.segs[g].first_ent = j;
  }
  for (uint64_t c = 0; c < n; ++c)
    if (mark[c]) r.segs[seg1[c] - 1].first_cmd = c, r.segs[seg1[c] - 1].mem_bytes = byt[c];
  if (closed) r.segs[nseg] = {n, (uint64_t)r.ents.size(), 0};
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
  for (const lsmck_wal_cmd& e : got.ents) CHECK(e.type == 1u && e.reserved == 0u);
  CHECK(got.nlong == want.nlong);
}

int main() {
  // the rules by themselves
  {
    lsmck_wal_cmd c{};
    c.type = 1, c.klen = 0xFFFFFFFFu - 8, c.vlen = 0;
    CHECK(wpl::fits(c));
    c.vlen = 1;
    CHECK(!wpl::fits(c));
    c.type = 2, c.vlen = 0;  // a delete's value is one byte
    CHECK(!wpl::fits(c));
    c.klen -= 1;
    CHECK(wpl::fits(c) && wpl::a_of(wpl::pack(c)) == 0xFFFFFFFFull - 9 + 1 && !wpl::is_insert(wpl::pack(c)));
    const uint8_t z[2] = {0, 7};
    CHECK(!wpl::tomb_bad(z, 2, 0) && wpl::tomb_bad(z, 2, 1) && wpl::tomb_bad(z, 2, 2) && wpl::tomb_bad(z, 0, 0));
    CHECK(wpl::qualifies(wpl::kInsertBit | 3, 5, 5) && !wpl::qualifies(3, 5, 5));
    CHECK(!wpl::qualifies(wpl::kInsertBit, 4, 5));
    CHECK(wpl::qualifies(wpl::kInsertBit, 0, 0) && !wpl::qualifies(wpl::kInsertBit, ~0ull - 1, ~0ull));
  }
  // the plan's two options: their defaults and ranges, looked up behind the main table
  {
    lsmck_host::Options o{};
    const lsmck_host::OptionEnv env{256, false};
    std::string why;
    CHECK(o.cut_walk_cap == 4096 && o.cut_block == 8192);
    auto set = [&](const char* key, long v) { return lsmck_host::option_set(o, key, v, env, &why); };
    for (long v : {1l, 4l, 4096l, 1l << 30}) CHECK(set("cut_walk_cap", v) == 0 && o.cut_walk_cap == v);
    for (long v : {0l, -1l, (1l << 30) + 1})
      CHECK(set("cut_walk_cap", v) == LSMCK_EINVAL && o.cut_walk_cap == 1l << 30);
    for (long v : {64l, 65l, 8192l}) CHECK(set("cut_block", v) == 0 && o.cut_block == v);
    for (long v : {0l, 63l, 8193l}) CHECK(set("cut_block", v) == LSMCK_EINVAL && o.cut_block == 8192);
    CHECK(why.find("cut_block") != std::string::npos);
    CHECK(lsmck_host::option_set(o, "mem_build_time", 1, env, &why) == 0 && o.mem_build_time == 1);
    CHECK(lsmck_host::option_set(o, "cut_nothing", 1, env, &why) == LSMCK_EINVAL);
  }
  const uint64_t limits[] = {0, 1, 7, 20, 64, 300, ~0ull};
  const uint32_t caps[] = {1, 2, 3, 4, 7, 64, 4096};
  const uint32_t blocks[] = {1, 2, 3, 5, 8, 64, 8192};
  size_t runs = 0;
  for (size_t n : {0, 1, 2, 3, 5, 17, 64, 65, 200, 513}) {
    for (int rep = 0; rep < (n < 100 ? 6 : 2); ++rep) {
      Stream s;
      make(s, n, 1 + rnd(n < 4 ? 3 : n / 2 + 1), rep % 2 ? 12 : 3, rep % 3 == 2 ? 2 : 6);
      for (uint64_t limit : limits)
        for (uint32_t cap : caps) {
          const uint32_t B = blocks[rnd(7)], width = (uint32_t)(1 + rnd(9));
          compare(s, limit, cap, B, width);
          ++runs;
        }
      for (uint32_t B : blocks) compare(s, 20, 3, B, 1024), ++runs;
    }
  }
  // only deletes; one key; a large value overwritten by a small one
  {
    Stream s;
    make(s, 100, 7, 5, 1);
    for (uint64_t limit : limits) compare(s, limit, 4, 8, 3), ++runs;
    Stream one;
    make(one, 150, 1, 12, 5);
    for (uint64_t limit : limits) compare(one, limit, 4, 8, 3), ++runs;
  }
  // memtables longer than two windows at the kernels' window (1024) and at 1000, in blocks of the widths the GPU
  // tests use: over a thousand keys, a limit that the first memtable reaches behind command 2100
  for (size_t n : {2500, 3100}) {
    Stream s;
    make(s, n, 1200, 12, 6, 26);
    uint64_t limit = 0;
    {
      std::map<std::string, uint64_t> mt;
      uint64_t bytes = 0;
      for (size_t i = 0; i <= 2100; ++i) {
        const lsmck_wal_cmd& c = s.cmds[i];
        const uint64_t a = (uint64_t)c.klen + wpl::ent_vlen(c);
        auto it = mt.find(s.key(c));
        if (it != mt.end()) bytes -= it->second;
        mt[s.key(c)] = a, bytes += a;
        limit = std::max(limit, bytes);
      }
    }
    const Result want = reference(s, limit, 64);
    g_what = "n " + std::to_string(n) + " limit " + std::to_string(limit);
    // the first memtable is closed in its third window
    CHECK(want.segs.size() >= 2 && want.segs[1].first_cmd > 2 * 1024 && want.nlong >= 1);
    for (uint64_t lim : {limit, (uint64_t)~0ull})
      for (uint32_t width : {1000u, 1024u})
        for (uint32_t B : {1024u, 1025u, 8192u})
          for (uint32_t cap : {4u, 64u, 4096u}) compare(s, lim, cap, B, width), ++runs;
  }
  printf("writeplan ok (%zu)\n", runs);
  return 0;
}
