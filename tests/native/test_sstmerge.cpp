// Host model of the batch SSTable decode and merge (csrc/lsmck_sstmerge.h): the
// steps the kernels of lsmck_sstmerge.hip run -- the record step, the index
// parse (serial, and item by item for keys of one length), the hint's acceptance rule, the order keys, the lower bound with its
// prefix fast path, the shadow, tombstone and slot rules -- table by table and
// entry by entry, compared with a restatement of the iterator that reads byte
// by byte and with a std::map updated in table order.  Built with
// -fsanitize=address,undefined: the arenas are exact-size heap blocks with
// tables flush against both ends (the merge's key arena 4-byte aligned and a
// multiple of 4 long: what a device allocation gives mem::chunk_tail), so a
// byte read outside an image is caught.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "lsmck_sstmerge.h"

using namespace lsmck;
typedef std::vector<std::pair<std::string, std::string>> Table;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

static int fails = 0;
#define CHECK(c, ...)                                 \
  do {                                                \
    if (!(c)) {                                       \
      printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
      printf(__VA_ARGS__);                            \
      printf("\n");                                   \
      if (++fails > 20) exit(1);                      \
    }                                                 \
  } while (0)

static void put(std::string& s, uint64_t x, int bytes) {
  for (int b = 0; b < bytes; ++b) s.push_back((char)(x >> (8 * b)));
}
// datafile.rs:27-35 and sstable_index.rs:42-46 (an item every `step` records)
static void encode(const Table& t, std::string* data, std::string* index, uint32_t step = 100) {
  std::string items;
  uint64_t count = 0;
  for (size_t i = 0; i < t.size(); ++i) {
    if (i % step == 0) {
      put(items, t[i].first.size(), 8);
      items += t[i].first;
      put(items, data->size(), 8);
      ++count;
    }
    put(*data, t[i].first.size(), 4);
    put(*data, t[i].second.size(), 4);
    *data += t[i].first + t[i].second;
  }
  put(*index, count, 8);
  *index += items;
}

// the iterator, byte by byte (sstable.rs:77-90, datafile.rs:60-83)
struct Rec {
  uint64_t key_pos, klen, vlen;
};
static std::vector<Rec> iterate(const std::string& img, uint64_t* consumed) {
  std::vector<Rec> out;
  uint64_t pos = 0;
  for (;;) {
    if (img.size() - pos < 8) break;  // read_u32 twice: UnexpectedEof
    uint64_t kl = 0, vl = 0;
    for (int b = 0; b < 4; ++b) kl |= (uint64_t)(uint8_t)img[pos + b] << (8 * b);
    for (int b = 0; b < 4; ++b) vl |= (uint64_t)(uint8_t)img[pos + 4 + b] << (8 * b);
    if (img.size() - pos - 8 < kl) break;       // read_exact(key)
    if (img.size() - pos - 8 - kl < vl) break;  // read_exact(val)
    out.push_back({pos + 8, kl, vl});
    pos += 8 + kl + vl;
  }
  *consumed = pos;
  return out;
}

struct Heap {  // an exact-size block
  uint8_t* p;
  size_t n;
  explicit Heap(const std::string& s) : n(s.size()) {
    p = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(p, s.data(), n);
  }
  ~Heap() { free(p); }
};

// ---- the decode, as the kernels run it ---------------------------------------
struct Decoded {
  std::vector<lsmck_wal_cmd> ents;
  std::vector<uint64_t> tab_first, consumed;
  uint64_t declined = 0, bad = ~0ull, uniform = 0, uniform_failed = 0;
};
static Decoded decode(const uint8_t* data, uint64_t db, const uint8_t* index, uint64_t ib,
                      const std::vector<lsmck_sstable_span>& spans) {
  const uint64_t ntab = spans.size(), nslots = index ? ib / 16 + ntab : 0;
  Decoded D;
  std::vector<uint64_t> segfirst(ntab + 1, 0), segpos(nslots + 1), cons(ntab, 0), cnt(ntab + 1, 0);
  std::vector<uint32_t> state(ntab), fail(ntab, 0), lastcnt(ntab, 0);
  for (uint64_t t = 0; t < ntab; ++t) {  // dec_index_count
    const lsmck_sstable_span s = spans[t];
    bool ok = mrg::span_ok(s.data_off, s.data_len, db) && s.data_len <= mrg::kMaxTable;
    if (index) ok = ok && mrg::span_ok(s.index_off, s.index_len, ib);
    if (!ok) {
      if (t < D.bad) D.bad = t;
      state[t] = 2, fail[t] = 2;
      continue;
    }
    if (!index) {
      state[t] = 2;
      continue;
    }
    uint64_t c, klen0;
    if (mrg::index_uniform(index + s.index_off, s.index_len, &c, &klen0)) {
      segfirst[t] = c, state[t] = 3;
      ++D.uniform;
      continue;
    }
    c = mrg::index_parse(index + s.index_off, s.index_len, s.data_len, nullptr, 0);
    if (c == ~0ull) state[t] = 1;
    else if (c == 0) state[t] = mrg::empty_check(data + s.data_off, s.data_len) ? 0 : 1;
    else segfirst[t] = c, state[t] = 0;
  }
  uint64_t acc = 0;
  for (uint64_t t = 0; t <= ntab; ++t) {
    const uint64_t c = t < ntab ? segfirst[t] : 0;
    segfirst[t] = acc;
    acc += c;
  }
  for (uint64_t sl = 0; sl < nslots && sl < segfirst[ntab]; ++sl) {  // dec_index_uniform
    const uint64_t t = mrg::table_of(segfirst.data(), ntab, sl);
    if (state[t] != 3) continue;
    const uint8_t* idx = index + spans[t].index_off;
    uint64_t p;
    if (mrg::uniform_item(idx, spans[t].data_len, mrg::load64(idx + 8), sl - segfirst[t], &p)) segpos[sl] = p;
    else fail[t] |= 1;
  }
  for (uint64_t t = 0; t < ntab; ++t) {  // dec_index_fill
    const uint64_t k = segfirst[t + 1] - segfirst[t];
    if ((state[t] != 0 && state[t] != 3) || k == 0) continue;
    if (segfirst[t + 1] > nslots) {
      state[t] = 1;
      continue;
    }
    std::vector<uint64_t> serial(k);
    const uint64_t c = mrg::index_parse(index + spans[t].index_off, spans[t].index_len, spans[t].data_len,
                                        serial.data(), k);
    if (state[t] == 3) {
      if (!(fail[t] & 1)) {  // every item checked: the serial parse says the same
        CHECK(c == k && std::equal(serial.begin(), serial.end(), segpos.begin() + segfirst[t]), "the parallel parse");
        continue;
      }
      fail[t] = 0;
      ++D.uniform_failed;
    } else {
      CHECK(c == k, "the second parse differs");
    }
    if (c != k) state[t] = 1;
    else std::copy(serial.begin(), serial.end(), segpos.begin() + segfirst[t]);
  }
  for (uint64_t sl = 0; sl < nslots && sl < segfirst[ntab]; ++sl) {  // dec_seg_check
    const uint64_t t = mrg::table_of(segfirst.data(), ntab, sl);
    if (state[t] != 0 && state[t] != 3) continue;
    const bool last = sl + 1 == segfirst[t + 1];
    uint32_t c;
    uint64_t end;
    if (!mrg::seg_check(data + spans[t].data_off, spans[t].data_len, segpos[sl], last, last ? 0 : segpos[sl + 1], &c,
                        &end))
      fail[t] |= 1;
    else if (last)
      lastcnt[t] = c, cons[t] = end;
  }
  std::vector<uint8_t> hint(ntab, 0);
  for (uint64_t t = 0; t < ntab; ++t) {  // dec_count
    if (fail[t] & 2) continue;
    const uint64_t k = segfirst[t + 1] - segfirst[t];
    if ((state[t] == 0 || state[t] == 3) && !fail[t]) {
      hint[t] = 1;
      cnt[t] = k ? (k - 1) * mrg::kStep + lastcnt[t] : 0;
      if (!k) cons[t] = 0;
      continue;
    }
    if (state[t] != 2) ++D.declined;
    uint64_t end;
    cnt[t] = mrg::walk(data + spans[t].data_off, spans[t].data_len, spans[t].data_off, 0, ~0ull, nullptr, &end);
    cons[t] = end;
  }
  acc = 0;
  for (uint64_t t = 0; t <= ntab; ++t) {
    const uint64_t c = t < ntab ? cnt[t] : 0;
    cnt[t] = acc;
    acc += c;
  }
  if (D.bad != ~0ull) return D;
  D.ents.resize(acc);
  for (uint64_t sl = 0; sl < nslots && sl < segfirst[ntab]; ++sl) {  // dec_emit_seg
    const uint64_t t = mrg::table_of(segfirst.data(), ntab, sl);
    if (!hint[t]) continue;
    const uint64_t e0 = cnt[t] + (sl - segfirst[t]) * mrg::kStep, room = cnt[t + 1] - e0;
    uint64_t end;
    (void)mrg::walk(data + spans[t].data_off, spans[t].data_len, spans[t].data_off, segpos[sl],
                    room < mrg::kStep ? room : mrg::kStep, D.ents.data() + e0, &end);
  }
  for (uint64_t t = 0; t < ntab; ++t) {  // dec_emit_plain
    if (hint[t]) continue;
    uint64_t end;
    (void)mrg::walk(data + spans[t].data_off, spans[t].data_len, spans[t].data_off, 0, cnt[t + 1] - cnt[t],
                    D.ents.data() + cnt[t], &end);
  }
  D.tab_first = cnt;
  D.consumed = cons;
  return D;
}

// images back to back in exact-size arenas, decoded with and without the index
static Decoded check_decode(const char* what, const std::vector<std::string>& datas,
                            const std::vector<std::string>& idxs, uint64_t want_declined) {
  Decoded with_index;
  std::string da, ia;
  std::vector<lsmck_sstable_span> spans;
  for (size_t t = 0; t < datas.size(); ++t) {
    spans.push_back({da.size(), datas[t].size(), ia.size(), idxs[t].size()});
    da += datas[t], ia += idxs[t];
  }
  const Heap hd(da), hi(ia);
  for (int with = 0; with < 2; ++with) {
    const Decoded D = decode(hd.p, hd.n, with ? hi.p : nullptr, hi.n, spans);
    CHECK(D.bad == ~0ull, "%s", what);
    CHECK(D.declined == (with ? want_declined : 0), "%s: %llu declined, expected %llu", what,
          (unsigned long long)D.declined, (unsigned long long)(with ? want_declined : 0));
    uint64_t e = 0;
    for (size_t t = 0; t < datas.size(); ++t) {
      uint64_t consumed;
      const std::vector<Rec> want = iterate(datas[t], &consumed);
      CHECK(D.tab_first[t] == e && D.consumed[t] == consumed, "%s: table %zu", what, t);
      uint64_t c2 = 0;
      CHECK(mrg::walk((const uint8_t*)datas[t].data(), datas[t].size(), 0, 0, ~0ull, nullptr, &c2) == want.size() &&
                c2 == consumed, "%s: count", what);
      for (const Rec& r : want) {
        if (e >= D.ents.size()) break;
        const lsmck_wal_cmd c = D.ents[e++];
        CHECK(c.key_off == spans[t].data_off + r.key_pos && c.klen == r.klen && c.vlen == r.vlen &&
                  c.val_off == c.key_off + r.klen && c.type == 1 && c.reserved == 0, "%s: table %zu entry", what, t);
      }
    }
    CHECK(e == D.ents.size() && D.tab_first.back() == e, "%s: %llu entries", what, (unsigned long long)e);
    if (with) with_index = D;
  }
  return with_index;
}

static Table make_table(uint32_t m, uint32_t seed) {
  Table t;
  for (uint32_t i = 0; i < m; ++i) {
    char k[32];
    snprintf(k, sizeof k, "%c%06u", 'a' + (char)(seed % 20), i);
    std::string key(k, i % 7 == 3 ? 0 : 1 + (i + seed) % 7);  // (order does not matter to the decode)
    key += std::string(k);
    if (i == 0 && seed % 3 == 0) key.clear();
    t.push_back({key, std::string((i * 7 + seed) % 23, (char)('A' + i % 26))});
  }
  return t;
}

// keys of one length: the index is proven item by item
static Table fixed_table(uint32_t m, uint32_t seed) {
  Table t;
  for (uint32_t i = 0; i < m; ++i) {
    char k[32];
    snprintf(k, sizeof k, "%c%011u", 'a' + (char)(seed % 20), i);
    t.push_back({std::string(k, 12), std::string((i * 5 + seed) % 17, 'v')});
  }
  return t;
}

static void test_decode_uniform() {
  for (uint32_t m : {1u, 100u, 101u, 250u, 1000u}) {
    std::string d, x;
    encode(fixed_table(m, m), &d, &x);
    const Decoded D = check_decode("fixed keys", {d, d}, {x, x}, 0);
    CHECK(D.uniform == 2 && D.uniform_failed == 0, "fixed keys: %llu", (unsigned long long)D.uniform);
  }
  {  // item keys of 6, 4 and 8 bytes: the lengths add up as three of 6 would, the items are not where those would be
    Table t = fixed_table(250, 1);
    t[0].first = "a00000", t[100].first = "a100", t[200].first = "a2000000";
    std::string d, x;
    encode(t, &d, &x);
    const Decoded D = check_decode("a coincidence", {d}, {x}, 0);
    CHECK(D.uniform == 1 && D.uniform_failed == 1, "a coincidence");
  }
  {  // damaged, keys of one length
    std::string d, x;
    const Table t = fixed_table(250, 2);
    encode(t, &d, &x);
    const size_t pos1 = 8 + 28 + 8 + 12;
    auto add = [&](size_t at, int64_t delta) {
      std::string y = x;
      uint64_t v;
      memcpy(&v, &y[at], 8);
      v += (uint64_t)delta;
      memcpy(&y[at], &v, 8);
      return y;
    };
    check_decode("fixed pos + 1", {d, d}, {add(pos1, 1), x}, 1);
    check_decode("fixed pos_0", {d}, {add(8 + 20, 3)}, 1);
    check_decode("fixed order", {d}, {add(pos1, 1 << 20)}, 1);
    check_decode("fixed klen", {d}, {add(8 + 28, 1)}, 1);
    check_decode("fixed count", {d}, {add(0, 1)}, 1);
    std::string d50, x50;
    encode(t, &d50, &x50, 50);
    check_decode("fixed step 50", {d}, {x50}, 1);
  }
}

static void test_decode() {
  const uint32_t sizes[] = {0, 1, 2, 99, 100, 101, 199, 200, 201, 250, 1000};
  // every size, alone and flush against both ends of the arena
  for (uint32_t m : sizes) {
    std::string d, x;
    encode(make_table(m, m), &d, &x);
    check_decode("one table", {d}, {x}, 0);
  }
  {  // many tables, all sizes, at every residue
    std::vector<std::string> ds, xs;
    for (uint32_t r = 0; r < 40; ++r) {
      std::string d, x;
      encode(make_table(sizes[r % 11] + r % 3, r), &d, &x);
      ds.push_back(d), xs.push_back(x);
    }
    check_decode("many tables", ds, xs, 0);
  }
  // every cut of the last record: the index of the uncut table is refused
  // only where its last segment's count changes nothing it checks
  for (uint32_t m : {1u, 100u, 101u, 201u}) {
    std::string d, x;
    const Table t = make_table(m, 5);
    encode(t, &d, &x);
    const uint64_t last = 8 + t.back().first.size() + t.back().second.size();
    for (uint64_t cut = 1; cut <= last; ++cut) {
      const std::string dc = d.substr(0, d.size() - cut);
      // the index built for the cut table's whole records
      std::string d2, x2;
      encode(Table(t.begin(), t.end() - 1), &d2, &x2);
      check_decode("cut tail", {dc, d}, {x2, x}, 0);
      // the uncut table's index over the cut image: usable unless the cut record was an item's
      check_decode("cut tail, old index", {dc}, {x}, (m - 1) % 100 == 0 ? 1 : 0);
    }
  }
  // damaged indexes: refused, the entries unchanged
  {
    std::string d, x;
    const Table t = make_table(250, 9);
    encode(t, &d, &x);
    auto u64_at = [&](std::string& s, size_t at, int64_t delta) {
      uint64_t v;
      memcpy(&v, &s[at], 8);
      v += (uint64_t)delta;
      memcpy(&s[at], &v, 8);
    };
    const size_t k0 = t[0].first.size(), k1 = t[100].first.size();
    const size_t pos0 = 8 + 8 + k0, pos1 = pos0 + 8 + 8 + k1;
    std::string y;
    y = x, u64_at(y, pos1, 1), check_decode("pos + 1", {d}, {y}, 1);
    y = x, u64_at(y, pos1, -1), check_decode("pos - 1", {d}, {y}, 1);
    y = x, u64_at(y, 0, 1), check_decode("count + 1", {d}, {y}, 1);
    y = x, u64_at(y, 0, -1), check_decode("count - 1", {d}, {y}, 1);
    y = x.substr(0, x.size() - 1), check_decode("truncated", {d}, {y}, 1);
    y = x.substr(0, 7), check_decode("truncated count", {d}, {y}, 1);
    y = x + "z", check_decode("trailing", {d}, {y}, 1);
    y = x, u64_at(y, pos0, 8), check_decode("pos_0 != 0", {d}, {y}, 1);
    y = x, u64_at(y, pos1, 1 << 20), check_decode("past data_len", {d}, {y}, 1);
    {
      y = x;
      const size_t pos2 = pos1 + 8 + 8 + t[200].first.size();
      uint64_t a, b;
      memcpy(&a, &y[pos1], 8), memcpy(&b, &y[pos2], 8);
      memcpy(&y[pos1], &b, 8), memcpy(&y[pos2], &a, 8);
      check_decode("out of order", {d}, {y}, 1);
    }
    y = x, u64_at(y, 8, 1ll << 40), check_decode("huge klen", {d}, {y}, 1);
    {
      std::string d50, x50;
      encode(t, &d50, &x50, 50);
      check_decode("step 50", {d}, {x50}, 1);
    }
    {  // an empty table whose index names records, a full one whose index is empty
      std::string none;
      put(none, 0, 8);
      check_decode("empty index over records", {d}, {none}, 1);
      check_decode("index over an empty table", {std::string()}, {x}, 1);
      check_decode("three bytes", {std::string("abc")}, {none}, 0);
    }
    // among good tables only the damaged one is walked plainly
    y = x, u64_at(y, pos1, 1);
    check_decode("one of three", {d, d, d}, {x, y, x}, 1);
  }
  // spans outside the arena
  {
    std::string d, x;
    encode(make_table(3, 1), &d, &x);
    const Heap hd(d), hi(x);
    std::vector<lsmck_sstable_span> sp = {{0, d.size(), 0, x.size()}, {1, d.size(), 0, x.size()}};
    CHECK(decode(hd.p, hd.n, hi.p, hi.n, sp).bad == 1, "span");
    sp[1] = {0, d.size(), 1, x.size()};
    CHECK(decode(hd.p, hd.n, hi.p, hi.n, sp).bad == 1, "index span");
    CHECK(decode(hd.p, hd.n, nullptr, 0, sp).bad == ~0ull, "index span without an index");
    sp[0] = {~0ull, 2, 0, 0};
    CHECK(decode(hd.p, hd.n, nullptr, 0, sp).bad == 0, "wrapping span");
  }
}

// ---- the merge, as the kernels run it ------------------------------------------
struct Merged {
  std::vector<uint32_t> src;
  std::vector<uint64_t> out_first;
  uint64_t bad = ~0ull, stuck = ~0ull;
};
static Merged merge(const uint8_t* keys, uint64_t kb, const std::vector<lsmck_wal_cmd>& ents,
                    const std::vector<uint64_t>& tf, const std::vector<uint64_t>& gf, uint32_t mode) {
  const uint64_t n = ents.size(), ntab = tf.size() - 1, ngrp = gf.size() - 1;
  Merged M;
  M.out_first.assign(ngrp + 1, 0);
  if (!n) return M;
  std::vector<uint32_t> tgrp(ntab), etab(n);
  for (uint64_t g = 0; g < ngrp; ++g)
    for (uint64_t t = gf[g]; t < gf[g + 1]; ++t) tgrp[t] = (uint32_t)g;
  std::vector<mrg::OKey> ok(n);
  for (uint64_t i = 0; i < n; ++i) {  // mrg_okey
    etab[i] = (uint32_t)mrg::table_of(tf.data(), ntab, i);
    CHECK(tf[etab[i]] <= i && i < tf[etab[i] + 1], "table_of");
    ok[i] = mrg::OKey{0, 0, 0};
    if (sst::rec_size(ents[i], kb, kb)) ok[i] = mrg::okey_of(keys, ents[i]);
    else if (i < M.bad) M.bad = i;
  }
  for (uint64_t i = 1; i < n; ++i) {  // mrg_order
    if (etab[i] != etab[i - 1]) continue;
    const lsmck_wal_cmd a = ents[i - 1], b = ents[i];
    if (!sst::rec_size(a, kb, kb) || !sst::rec_size(b, kb, kb)) continue;
    if (!sst::key_less(keys + a.key_off, a.klen, keys + b.key_off, b.klen) && i < M.bad) M.bad = i;
  }
  if (M.bad != ~0ull) return M;
  std::vector<uint64_t> lp(n + 1, 0);
  std::vector<uint8_t> tomb(n, 0);
  for (uint64_t i = 0; i < n; ++i) {  // mrg_shadow
    const uint64_t t = etab[i];
    const bool sh = mrg::shadowed(ok.data(), ents.data(), keys, tf.data(), t, gf[tgrp[t] + 1], i);
    const bool tb = !sh && mode != 2 && mrg::tombstone(ents[i], keys);
    lp[i] = !sh && !(tb && mode == 1);
    tomb[i] = tb && mode == 0;
  }
  uint64_t acc = 0;
  for (uint64_t i = 0; i <= n; ++i) {
    const uint64_t c = i < n ? lp[i] : 0;
    lp[i] = acc;
    acc += c;
  }
  for (uint64_t i = 0; i < n; ++i) {  // mrg_stuck
    if (!tomb[i]) continue;
    const uint64_t t = etab[i], g = tgrp[t];
    const uint64_t w = (mrg::slot_of(ok.data(), ents.data(), keys, tf.data(), lp.data(), gf[g], gf[g + 1], t, i) << 32) | i;
    if (w < M.stuck) M.stuck = w;
  }
  for (uint64_t g = 0; g <= ngrp; ++g) M.out_first[g] = lp[tf[gf[g]]];
  if (M.stuck != ~0ull) {
    M.stuck &= 0xFFFFFFFFull;
    return M;
  }
  M.src.assign(acc, 0xFFFFFFFFu);
  for (uint64_t i = 0; i < n; ++i) {  // mrg_place
    if (lp[i + 1] == lp[i]) continue;
    const uint64_t t = etab[i], g = tgrp[t];
    const uint64_t s = mrg::slot_of(ok.data(), ents.data(), keys, tf.data(), lp.data(), gf[g], gf[g + 1], t, i);
    CHECK(s < acc && M.src[s] == 0xFFFFFFFFu, "slot %llu taken twice or out of range", (unsigned long long)s);
    if (s < acc) M.src[s] = (uint32_t)i;
  }
  return M;
}

// groups of tables (each a std::map: strictly increasing) against a std::map updated in table order
static void check_merge(const char* what, const std::vector<std::vector<std::map<std::string, std::string>>>& groups) {
  std::string arena;
  std::vector<lsmck_wal_cmd> ents;
  std::vector<uint64_t> tf{0}, gf{0};
  for (auto& g : groups) {
    for (auto& t : g) {
      for (auto& kv : t) {
        put(arena, kv.first.size(), 4), put(arena, kv.second.size(), 4);
        ents.push_back(mrg::entry_of(0, arena.size() - 8, (uint32_t)kv.first.size(), (uint32_t)kv.second.size()));
        arena += kv.first + kv.second;
      }
      tf.push_back(ents.size());
    }
    gf.push_back(tf.size() - 1);
  }
  // the arena ends with its last value; a multiple of 4 long, 4-byte aligned (mem::chunk_tail's contract)
  if (arena.size() % 4) {
    arena.append(4 - arena.size() % 4, '\xEE');
  }
  uint8_t* keys = nullptr;
  if (posix_memalign((void**)&keys, sizeof(void*), arena.size() ? arena.size() : 4)) abort();
  memcpy(keys, arena.data(), arena.size());
  for (uint32_t mode = 0; mode < 3; ++mode) {
    const Merged M = merge(keys, arena.size(), ents, tf, gf, mode);
    CHECK(M.bad == ~0ull, "%s: sorted tables refused", what);
    std::vector<uint32_t> want;
    std::vector<uint64_t> first{0};
    uint64_t stuck = ~0ull, e0 = 0;
    for (auto& g : groups) {
      std::map<std::string, uint32_t> m;
      uint64_t e = e0;
      for (auto& t : g)
        for (auto& kv : t) m[kv.first] = (uint32_t)e++;
      e0 = e;
      for (auto& kv : m) {
        const lsmck_wal_cmd c = ents[kv.second];
        const bool tb = c.vlen == 1 && keys[c.val_off] == 0;
        if (tb && mode == 0 && stuck == ~0ull) stuck = kv.second;
        if (tb && mode == 1) continue;
        want.push_back(kv.second);
      }
      first.push_back(want.size());
    }
    if (mode == 0 && stuck != ~0ull) {
      CHECK(M.stuck == stuck, "%s: stuck at %llu, expected %llu", what, (unsigned long long)M.stuck,
            (unsigned long long)stuck);
      continue;
    }
    CHECK(M.stuck == ~0ull, "%s: stuck", what);
    CHECK(M.src == want, "%s mode %u: %zu winners, expected %zu", what, mode, M.src.size(), want.size());
    CHECK(M.out_first == first, "%s: out_first", what);
  }
  free(keys);
}

static std::string key_from_pool(uint32_t i) {
  // ties through 7, 8, 9 and 16 bytes, proper prefixes at 7, 8 and 9, bytes >= 0x80, 00 01 against 01 00
  static const char* base = "ABCDEFGHIJKLMNOPQRSTUVWX";
  switch (i % 16) {
    case 0: return std::string();
    case 1: return std::string(base, 7);
    case 2: return std::string(base, 8);
    case 3: return std::string(base, 9);
    case 4: return std::string(base, 7) + "\x80";
    case 5: return std::string(base, 8) + "\xFF";
    case 6: return std::string(base, 9) + std::string(1, '\0');
    case 7: return std::string(base, 16);
    case 8: return std::string(base, 16) + "a";
    case 9: return std::string(base, 16) + "b";
    case 10: return std::string("\x00\x01", 2);
    case 11: return std::string("\x01\x00", 2);
    case 12: return std::string(base, 8) + std::string(1, '\0');
    case 13: return std::string(1, '\0');
    case 14: return std::string(base, 20) + std::string(below(46), 'z');
    default: return std::string(1 + below(20), (char)(0x7E + below(4)));
  }
}
static std::string value_from_pool() {
  switch (below(6)) {
    case 0: return std::string(1, '\0');
    case 1: return std::string(2, '\0');
    case 2: return std::string("\x01");
    case 3: return std::string();
    default: return std::string(1 + below(9), (char)('a' + below(26)));
  }
}

static void test_merge() {
  typedef std::map<std::string, std::string> T;
  check_merge("nothing", {});
  check_merge("an empty group", {{}});
  check_merge("empty tables", {{T{}, T{}}});
  check_merge("one table", {{T{{"a", "1"}, {"b", "2"}}}});
  check_merge("identical", {{T{{"a", "1"}, {"b", "2"}}, T{{"a", "3"}, {"b", "4"}}}});
  check_merge("disjoint", {{T{{"c", "1"}, {"d", "2"}}, T{{"a", "3"}, {"b", "4"}}}});
  check_merge("tombstone wins", {{T{{"a", "1"}}, T{{"a", std::string(1, '\0')}, {"b", "x"}}}});
  check_merge("tombstone shadowed", {{T{{"a", std::string(1, '\0')}}, T{{"a", "1"}}}});
  check_merge("tombstone first and last",
              {{T{{"a", std::string(1, '\0')}, {"m", "1"}}, T{{"z", std::string(1, '\0')}}}, {T{{"b", "1"}}}});
  check_merge("second group sticks", {{T{{"b", "1"}}}, {}, {T{{"a", std::string(1, '\0')}}}});
  for (uint32_t round = 0; round < 300; ++round) {
    std::vector<std::vector<T>> groups(1 + below(4));
    for (auto& g : groups) {
      g.resize(below(8));
      for (auto& t : g)
        for (uint32_t c = below(below(3) ? 12 : 40); c; --c) t[key_from_pool(below(64))] = value_from_pool();
    }
    check_merge("random", groups);
  }
  // the validation: an unsorted table and a repeated key
  {
    const std::string arena = "bbaaccxx";
    uint8_t* keys;
    if (posix_memalign((void**)&keys, sizeof(void*), 8)) abort();
    memcpy(keys, arena.data(), 8);
    auto e = [](uint64_t off, uint32_t kl) { lsmck_wal_cmd c{off, 6, kl, 1, 1, 0}; return c; };
    std::vector<lsmck_wal_cmd> ents{e(2, 2), e(0, 2), e(4, 2), e(4, 2), e(2, 2)};
    CHECK(merge(keys, 8, ents, {0, 2, 5}, {0, 2}, 2).bad == 3, "a repeated key");
    CHECK(merge(keys, 8, ents, {0, 1, 5}, {0, 2}, 2).bad == 3, "a repeated key in the second table");
    CHECK(merge(keys, 8, ents, {0, 1, 3, 4, 5}, {0, 4}, 2).bad == ~0ull, "tables of one");
    CHECK(merge(keys, 8, ents, {0, 1, 3, 5}, {0, 3}, 2).bad == 4, "an unsorted table");
    ents[1].klen = 9;  // outside the arena
    CHECK(merge(keys, 8, ents, {0, 1, 3, 4, 5}, {0, 4}, 2).bad == 1, "a range outside the arena");
    ents[1].klen = 2, ents[0].type = 2;
    CHECK(merge(keys, 8, ents, {0, 1, 3, 4, 5}, {0, 4}, 2).bad == 0, "a type");
    free(keys);
  }
}

// the lower bound against a linear scan, keys tied through their first 8 bytes and beyond
static void test_lower_bound() {
  std::map<std::string, int> pool;
  for (uint32_t i = 0; i < 64; ++i) pool[key_from_pool(i)] = 0;
  std::string arena;
  std::vector<lsmck_wal_cmd> ents;
  for (auto& kv : pool) {
    ents.push_back(mrg::entry_of(0, arena.size(), (uint32_t)kv.first.size(), 0));
    ents.back().key_off -= 8;
    arena += kv.first;
  }
  arena.append((4 - arena.size() % 4) % 4, '\0');
  uint8_t* keys;
  if (posix_memalign((void**)&keys, sizeof(void*), arena.size())) abort();
  memcpy(keys, arena.data(), arena.size());
  std::vector<mrg::OKey> ok;
  for (auto& c : ents) ok.push_back(mrg::okey_of(keys, c));
  const uint64_t n = ents.size();
  for (uint64_t lo = 0; lo <= n; lo += 3)
    for (uint64_t hi = lo; hi <= n; hi += 5)
      for (uint64_t q = 0; q < n; ++q) {
        bool eq;
        const uint64_t lb = mrg::lower_bound(ok.data(), ents.data(), keys, lo, hi, ok[q], ents[q].key_off, &eq);
        uint64_t want = lo;
        while (want < hi && want < q) ++want;  // (the pool is sorted and distinct)
        CHECK(lb == want && eq == (want < hi && want == q), "lower bound [%llu, %llu) of %llu", (unsigned long long)lo,
              (unsigned long long)hi, (unsigned long long)q);
      }
  for (uint64_t a = 0; a < n; ++a)
    for (uint64_t b = 0; b < n; ++b) {
      const int c = mrg::okey_cmp(ok[a], ents[a].key_off, ok[b], ents[b].key_off, keys);
      CHECK((c < 0) == (a < b) && (c > 0) == (a > b), "okey_cmp %llu %llu", (unsigned long long)a, (unsigned long long)b);
    }
  free(keys);
}

int main() {
  test_decode();
  test_decode_uniform();
  test_lower_bound();
  test_merge();
  if (fails) return printf("%d checks failed\n", fails), 1;
  printf("sstmerge ok\n");
  return 0;
}
