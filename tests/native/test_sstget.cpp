// Host model of the batch point read (csrc/lsmck_sstget.h): the steps the
// kernels of lsmck_sstget.hip run -- the spans' check and the item count, the
// item offsets (in place for an index of one key length, by the serial parse
// otherwise), the order keys with the order check, the queries' check, every
// (query, table) pair with the winner's minimum, resolve -- in the kernels'
// order, compared with a model that parses the index byte by byte into a
// std::map and runs SsTable::get's two branches as loops over bytes.  Built
// with -fsanitize=address,undefined: the data and index arenas are exact-size
// heap blocks with tables flush against both ends, and the query keys end
// flush with their block (its start 4-byte aligned and its length a multiple
// of 4: what a device allocation gives mem::chunk_tail), so a byte read
// outside an image is caught.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "lsmck_sstget.h"

using namespace lsmck;
typedef std::vector<std::pair<std::string, std::string>> Entries;

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

static int fails = 0;
#define CHECK(c, ...)                                    \
  do {                                                   \
    if (!(c)) {                                          \
      printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
      printf(__VA_ARGS__);                               \
      printf("\n");                                      \
      if (++fails > 20) exit(1);                         \
    }                                                    \
  } while (0)

static void put(std::string& s, uint64_t x, int bytes) {
  for (int b = 0; b < bytes; ++b) s.push_back((char)(x >> (8 * b)));
}
static std::string data_image(const Entries& t, std::vector<uint64_t>* pos = nullptr) {
  std::string d;
  for (auto& e : t) {
    if (pos) pos->push_back(d.size());
    put(d, e.first.size(), 4);
    put(d, e.second.size(), 4);
    d += e.first + e.second;
  }
  return d;
}
typedef std::vector<std::pair<std::string, uint64_t>> Items;
static std::string items_image(const Items& items) {
  std::string x;
  put(x, items.size(), 8);
  for (auto& it : items) {
    put(x, it.first.size(), 8);
    x += it.first;
    put(x, it.second, 8);
  }
  return x;
}
static Items items_of(const Entries& t, uint32_t step) {
  std::vector<uint64_t> pos;
  (void)data_image(t, &pos);
  Items items;
  for (size_t i = 0; i < t.size(); i += step) items.push_back({t[i].first, pos[i]});
  return items;
}

// ---- the model: a std::map and loops over bytes --------------------------------
static uint64_t rd(const std::string& s, uint64_t at, int bytes) {
  uint64_t v = 0;
  for (int b = 0; b < bytes; ++b) v |= (uint64_t)(uint8_t)s[at + b] << (8 * b);
  return v;
}
struct RefMap {
  bool ok = false;
  std::map<std::string, uint64_t> m;
};
static RefMap ref_map(const std::string& x) {
  RefMap R;
  if (x.size() < 8) return R;
  const uint64_t count = rd(x, 0, 8);
  uint64_t at = 8;
  std::string prev;
  for (uint64_t j = 0; j < count; ++j) {
    if (x.size() - at < 8) return R;
    const uint64_t kl = rd(x, at, 8);
    if (x.size() - at - 8 < kl || x.size() - at - 8 - kl < 8) return R;
    const std::string key = x.substr(at + 8, kl);
    if (j && !(prev < key)) return R;  // (std::string compares as unsigned bytes, a proper prefix first)
    R.m[key] = rd(x, at + 8 + kl, 8);
    prev = key;
    at += 16 + kl;
  }
  R.ok = at == x.size();
  return R;
}
struct RefRec {
  uint64_t kpos, klen, vlen, size;
};
static bool ref_read(const std::string& d, uint64_t pos, RefRec* r) {  // datafile.rs:60-83
  if (pos > d.size() || d.size() - pos < 8) return false;
  const uint64_t kl = rd(d, pos, 4), vl = rd(d, pos + 4, 4);
  if (d.size() - pos - 8 < kl || d.size() - pos - 8 - kl < vl) return false;
  *r = {pos + 8, kl, vl, 8 + kl + vl};
  return true;
}
static bool ref_get(const std::string& d, const RefMap& R, const std::string& key, uint64_t* vpos, uint64_t* vlen) {
  RefRec r;
  auto hit = R.m.find(key);
  if (hit != R.m.end()) {
    if (!ref_read(d, hit->second, &r)) return false;
    *vpos = r.kpos + r.klen, *vlen = r.vlen;
    return true;
  }
  auto lb = R.m.lower_bound(key);
  uint64_t pos = lb == R.m.begin() ? 0 : std::prev(lb)->second;
  const uint64_t end = lb == R.m.end() ? d.size() : lb->second;
  while (ref_read(d, pos, &r)) {
    if (r.klen == key.size() && d.compare(r.kpos, r.klen, key) == 0) {
      *vpos = r.kpos + r.klen, *vlen = r.vlen;
      return true;
    }
    pos += r.size;
    if (pos >= end) break;
  }
  return false;
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

// ---- the call, as the kernels run it ---------------------------------------------
struct Batch {
  std::vector<std::pair<std::string, std::string>> tables;  // (data, index) in search order
  std::vector<lsmck_sstable_span> spans;
  std::string data, index, qkeys;
  std::vector<lsmck_get_query> q;
  std::vector<std::string> keys;
  void add_table(const std::string& d, const std::string& x) {
    spans.push_back({data.size(), d.size(), index.size(), x.size()});
    data += d, index += x;
    tables.push_back({d, x});
  }
  void front(size_t n) { data.assign(n, (char)0xEE); }
  void set_keys(const std::vector<std::string>& ks) {
    keys = ks;
    size_t total = 0;
    for (auto& k : ks) total += k.size();
    qkeys.assign((4 - total % 4) % 4, (char)0xDD);  // the last key ends flush with a block of whole dwords
    q.clear();
    for (auto& k : ks) {
      q.push_back({qkeys.size(), (uint32_t)k.size(), 0u});
      qkeys += k;
    }
  }
};
struct Out {
  std::vector<lsmck_get_result> res;
  uint64_t bad_table = ~0ull, bad_query = ~0ull, total = 0, uniform_failed = 0, walked = 0, skipped = 0;
  bool regrow = false;
};
enum { kSerial = 0, kUniform = 1, kBad = 2 };

static Out run(const uint8_t* data, uint64_t db, const uint8_t* index, uint64_t ib,
               const std::vector<lsmck_sstable_span>& spans, const uint8_t* qkeys, uint64_t qb,
               const std::vector<lsmck_get_query>& q, uint64_t nslots, bool reversed) {
  const uint64_t ntab = spans.size(), n = q.size();
  Out O;
  std::vector<uint64_t> first(ntab + 1, 0), ioff(nslots + 1), ipos(nslots + 1);
  std::vector<mrg::OKey> iok(nslots + 1), qok(n);
  std::vector<uint32_t> state(ntab, 0), fail(ntab, 0), win(n);
  // 1. get_tab_count and the scan
  for (uint64_t t = 0; t < ntab; ++t) {
    const lsmck_sstable_span s = spans[t];
    uint64_t c = get::kNo, klen0;
    if (mrg::span_ok(s.data_off, s.data_len, db) && s.data_len <= mrg::kMaxTable &&
        mrg::span_ok(s.index_off, s.index_len, ib)) {
      if (mrg::index_uniform(index + s.index_off, s.index_len, &c, &klen0)) {
        first[t + 1] = c, state[t] = kUniform;
        continue;
      }
      c = get::index_parse(index + s.index_off, s.index_len, nullptr, 0);
    }
    if (c == get::kNo) {
      O.bad_table = std::min<uint64_t>(O.bad_table, t), state[t] = kBad;
      continue;
    }
    first[t + 1] = c, state[t] = kSerial;
  }
  for (uint64_t t = 0; t < ntab; ++t) first[t + 1] += first[t];
  O.total = first[ntab];
  if (O.total > nslots) {
    O.regrow = true;
    return O;
  }
  // 2a. get_items_uniform, 2b. get_items_fill
  for (uint64_t sl = 0; sl < O.total; ++sl) {
    const uint64_t t = mrg::table_of(first.data(), ntab, sl);
    if (state[t] != kUniform) continue;
    const uint8_t* idx = index + spans[t].index_off;
    const uint64_t klen0 = mrg::load64(idx + 8), j = sl - first[t];
    if (get::uniform_item(idx, klen0, j)) ioff[sl] = get::uniform_off(klen0, j);
    else fail[t] |= 1u;
  }
  for (uint64_t t = 0; t < ntab; ++t) {
    const uint64_t k = first[t + 1] - first[t];
    if (state[t] == kBad || k == 0) continue;
    if (state[t] == kUniform && !(fail[t] & 1u)) continue;
    if (state[t] == kUniform) ++O.uniform_failed;
    if (get::index_parse(index + spans[t].index_off, spans[t].index_len, ioff.data() + first[t], k) != k)
      O.bad_table = std::min<uint64_t>(O.bad_table, t), state[t] = kBad;
  }
  // 3. get_items_keys
  for (uint64_t sl = 0; sl < O.total; ++sl) {
    const uint64_t t = mrg::table_of(first.data(), ntab, sl);
    if (state[t] == kBad) continue;
    const uint8_t* idx = index + spans[t].index_off;
    iok[sl] = get::item_okey(idx, ioff[sl]);
    ipos[sl] = get::item_pos(idx, ioff[sl]);
    if (sl > first[t] && !get::item_less(idx, ioff[sl - 1], ioff[sl])) O.bad_table = std::min<uint64_t>(O.bad_table, t);
  }
  // 4a. get_queries
  for (uint64_t i = 0; i < n; ++i) {
    mrg::OKey k{0, 0, 0};
    if (get::query_ok(q[i], qb)) k = get::key_of(qkeys, q[i].key_off, q[i].klen).ok;
    else O.bad_query = std::min<uint64_t>(O.bad_query, i);
    qok[i] = k, win[i] = get::kNoTable;
  }
  if (O.bad_table != ~0ull || O.bad_query != ~0ull) return O;
  auto table = [&](uint64_t t) {
    get::Table T;
    T.img = data + spans[t].data_off, T.dlen = spans[t].data_len, T.idx = index + spans[t].index_off;
    T.ok = iok.data() + first[t], T.ioff = ioff.data() + first[t], T.ipos = ipos.data() + first[t];
    T.nitems = first[t + 1] - first[t];
    return T;
  };
  auto key = [&](uint64_t i) {
    get::Key k;
    k.p = q[i].klen ? qkeys + q[i].key_off : qkeys;
    k.ok = qok[i];
    return k;
  };
  // 4b. get_probe: the pairs in one order or the other -- the minimum must not depend on it
  const uint64_t total = n * ntab;
  for (uint64_t x = 0; x < total; ++x) {
    const uint64_t w = reversed ? total - 1 - x : x, t = w / n, i = w - t * n;
    if (t > win[i]) {
      ++O.skipped;
      continue;
    }
    uint64_t vpos;
    uint32_t vlen;
    bool walked;
    if (get::table_get(table(t), key(i), &vpos, &vlen, &walked)) win[i] = std::min<uint32_t>(win[i], (uint32_t)t);
    O.walked += walked;
  }
  // 5. get_resolve
  O.res.resize(n);
  for (uint64_t i = 0; i < n; ++i) {
    lsmck_get_result r = get::result_none();
    if (win[i] != get::kNoTable) {
      const get::Table T = table(win[i]);
      uint64_t vpos;
      uint32_t vlen;
      const bool some = get::table_get(T, key(i), &vpos, &vlen, nullptr);
      CHECK(some, "resolve finds what probe found (query %llu)", (unsigned long long)i);
      if (some) r = get::result_of(T.img, spans[win[i]].data_off, vpos, vlen, win[i]);
    }
    O.res[i] = r;
  }
  return O;
}

// the batch through exact-size blocks, both pair orders, against the model
static Out check(const Batch& b, const char* what, uint64_t want_bad_table = ~0ull, uint64_t want_bad_query = ~0ull,
                 const std::vector<lsmck_sstable_span>* spans_override = nullptr,
                 const std::vector<lsmck_get_query>* q_override = nullptr) {
  Heap D(b.data), X(b.index), K(b.qkeys);
  const std::vector<lsmck_sstable_span>& spans = spans_override ? *spans_override : b.spans;
  const std::vector<lsmck_get_query>& q = q_override ? *q_override : b.q;
  uint64_t nslots = b.index.size() / 16 + spans.size();
  Out O = run(D.p, D.n, X.p, X.n, spans, K.p, K.n, q, nslots, false);
  if (O.regrow) {
    CHECK(O.total > nslots, "%s: regrow only when the items do not fit", what);
    nslots = O.total;
    O = run(D.p, D.n, X.p, X.n, spans, K.p, K.n, q, nslots, false);
    CHECK(!O.regrow, "%s: the second pass fits", what);
    O.regrow = true;
  }
  CHECK(O.bad_table == want_bad_table, "%s: bad_table %llu, want %llu", what, (unsigned long long)O.bad_table,
        (unsigned long long)want_bad_table);
  if (want_bad_table == ~0ull)
    CHECK(O.bad_query == want_bad_query, "%s: bad_query %llu, want %llu", what, (unsigned long long)O.bad_query,
          (unsigned long long)want_bad_query);
  if (want_bad_table != ~0ull || want_bad_query != ~0ull) {
    CHECK(O.res.empty(), "%s: no result on an error", what);
    return O;
  }
  const Out R = run(D.p, D.n, X.p, X.n, spans, K.p, K.n, q, nslots, true);
  CHECK(R.res.size() == O.res.size() && (O.res.empty() || !memcmp(R.res.data(), O.res.data(), 16 * O.res.size())),
        "%s: the pairs' order changes nothing", what);
  std::vector<RefMap> maps;
  std::vector<std::string> datas;
  for (auto& s : spans) {
    datas.push_back(b.data.substr(s.data_off, s.data_len));
    maps.push_back(ref_map(b.index.substr(s.index_off, s.index_len)));
    CHECK(maps.back().ok, "%s: the model takes every index the call takes", what);
  }
  for (size_t i = 0; i < q.size(); ++i) {
    lsmck_get_result want = get::result_none();
    for (size_t t = 0; t < spans.size(); ++t) {
      uint64_t vpos, vlen;
      const std::string& d = datas[t];
      if (!ref_get(d, maps[t], b.keys[i], &vpos, &vlen)) continue;
      want.val_off = spans[t].data_off + vpos, want.vlen = (uint32_t)vlen, want.table = (uint32_t)t;
      if (vlen == 1 && d[vpos] == 0) want.val_off |= LSMCK_GET_TOMBSTONE;
      break;
    }
    const lsmck_get_result g = O.res[i];
    CHECK(g.val_off == want.val_off && g.vlen == want.vlen && g.table == want.table,
          "%s: query %zu: (%llx, %u, %u), want (%llx, %u, %u)", what, i, (unsigned long long)g.val_off, g.vlen, g.table,
          (unsigned long long)want.val_off, want.vlen, want.table);
  }
  return O;
}

// ---- cases ------------------------------------------------------------------------
static Entries make_table(uint32_t m, uint32_t seed, bool fixed) {
  Entries t;
  char buf[64];
  for (uint32_t i = 0; i < m; ++i) {
    std::string k, v;
    if (fixed) {
      snprintf(buf, sizeof buf, "%c%011u", 'a' + seed % 26, i * 3);
      k = buf;
    } else if (!(i == 0 && seed % 2 == 0)) {
      snprintf(buf, sizeof buf, "k%c%07u", 'A' + seed % 26, i * 3);
      k = std::string(buf) + std::string((i * 5 + seed) % 9, 'x');
    }
    if ((i + seed) % 11 == 3) v = "";
    else if ((i + seed) % 13 == 5) v = std::string(1, '\0');  // a tombstone
    else v = std::string((i * 7 + seed) % 19 + 1, (char)('0' + i % 10));
    t.push_back({k, v});
  }
  std::sort(t.begin(), t.end());
  return t;
}
static std::vector<std::string> queries_for(const std::vector<Entries>& tabs) {
  std::vector<std::string> ks = {"", std::string(19, (char)0xff), "k", "a"};
  for (auto& t : tabs)
    for (size_t i = 0; i < t.size(); ++i) {
      const std::string& k = t[i].first;
      ks.push_back(k);
      ks.push_back(k + std::string(1, '\0'));
      if (!k.empty()) {
        ks.push_back(k.substr(0, k.size() - 1));
        std::string lo = k;
        if ((uint8_t)lo.back() == 0) lo.pop_back();
        else lo.back() = (char)((uint8_t)lo.back() - 1), lo += "\xff\xff";
        ks.push_back(lo);
        if (i % 17 == 0) ks.push_back(k.substr(0, k.size() / 2));
      }
    }
  return ks;
}

static void test_sizes() {
  const uint32_t sizes[] = {0, 1, 99, 100, 101, 199, 200, 201, 350};
  for (uint32_t res = 0; res < 16; ++res) {
    Batch b;
    b.front(res);
    std::vector<Entries> tabs;
    for (uint32_t j = 0; j < 9; ++j) {
      const uint32_t m = sizes[(j + res) % 9];
      tabs.push_back(make_table(m, res + j, (res + j) % 3 == 0));
      b.add_table(data_image(tabs.back()), items_image(items_of(tabs.back(), 100)));
    }
    b.set_keys(queries_for(tabs));
    const Out O = check(b, "sizes");
    CHECK(O.walked > 0 && O.skipped > 0, "sizes: the probe walks and skips");
  }
}

static void test_ties() {
  const std::string B = "ABCDEFGHIJKLMNOPQRSTUVWX";
  std::vector<std::string> pool;
  for (size_t n = 0; n <= 20; ++n) pool.push_back(B.substr(0, n));
  for (int x : {0, 1, 0x7f, 0x80, 0xff})
    for (size_t n : {1, 2, 5, 9}) pool.push_back(B.substr(0, 8) + std::string(n, (char)x));
  for (int x = 0; x < 256; x += 15) pool.push_back(B.substr(0, 8) + "same-tail" + std::string(1, (char)x));
  for (int x : {0, 0x80, 0xff}) pool.push_back(std::string(8, (char)x)), pool.push_back(std::string(9, (char)x));
  std::sort(pool.begin(), pool.end());
  pool.erase(std::unique(pool.begin(), pool.end()), pool.end());
  Entries t;
  for (size_t i = 0; i < pool.size(); ++i) t.push_back({pool[i], "v" + std::to_string(i)});
  Entries ten;
  for (int a : {0, 1, 0x7f, 0x80, 0xff})
    for (int c = 0; c < 256; c += 17) ten.push_back({B.substr(0, 8) + std::string(1, (char)a) + std::string(1, (char)c), "f"});
  std::sort(ten.begin(), ten.end());
  const Entries pseudo = {{std::string(12, 'a'), "1"}, {std::string(11, 'b'), "2"}, {std::string(13, 'c'), "3"}};
  for (uint32_t step : {1u, 2u, 3u, 7u, 100u}) {
    Batch b;
    b.front(step);
    b.add_table(data_image(ten), items_image(items_of(ten, step)));
    b.add_table(data_image(t), items_image(items_of(t, step)));
    b.add_table(data_image(pseudo), items_image(items_of(pseudo, 1)));
    b.set_keys(queries_for({t, ten, pseudo}));
    const Out O = check(b, "ties");
    CHECK(O.uniform_failed == 1, "ties: the index of 12 + 11 + 13 key bytes is tried in place and parsed serially");
  }
}

static void test_doctored() {
  const Entries t = make_table(450, 7, false), f = make_table(450, 9, true);
  for (int round = 0; round < 36; ++round) {
    Batch b;
    b.front(below(16));
    for (const Entries* e : {&t, &f}) {
      Items items = items_of(*e, 100);
      std::vector<uint64_t> pos;
      const std::string d = data_image(*e, &pos);
      switch (round % 6) {
        case 0: items[1 + below(4)].second = pos[below(450)]; break;          // another record's position
        case 1: items[1 + below(4)].second = d.size() - below(12); break;     // at the end, or no header fits
        case 2: items[1 + below(4)].second = pos[below(450)] + 1 + below(7); break;  // mid-record
        case 3: items.erase(items.begin() + 1 + below(3)); break;              // an item missing
        case 4: std::swap(items[1].second, items[3].second); break;            // start >= end
        default: items[below(5)].second = rnd() | (1ull << 63); break;         // far past the end
      }
      b.add_table(d, items_image(items));
    }
    b.add_table(data_image(t), items_image(items_of(t, 100)));  // (a sound table behind them: it is asked next)
    b.set_keys(queries_for({t, f}));
    check(b, "doctored");
  }
}

static void test_cuts() {
  Entries e;
  for (int i = 0; i < 5; ++i) e.push_back({"c" + std::to_string(i) + std::string(i, 'y'), std::string(3 * i + 1, 'w')});
  std::vector<uint64_t> pos;
  const std::string d = data_image(e, &pos), x = items_image(items_of(e, 100));
  for (size_t cut = 0; cut <= d.size(); ++cut) {
    Batch b;
    b.add_table(d.substr(0, cut), x);
    b.set_keys(queries_for({e}));
    check(b, "cuts");
  }
}

static void test_refusals() {
  const Entries t = make_table(250, 1, false), f = make_table(450, 3, true);
  const Items it = items_of(t, 100), fi = items_of(f, 100);
  const std::string good = items_image(it), fgood = items_image(fi);
  auto count = [](std::string x, uint64_t c) {
    for (int b = 0; b < 8; ++b) x[b] = (char)(c >> (8 * b));
    return x;
  };
  std::string klen_off = fgood;
  klen_off[8 + 28] = 13;  // item 1's length: the image keeps the size of 5 items of one length
  const std::vector<std::string> bad = {
      good.substr(0, good.size() - 1), good + std::string(1, '\0'), count(good, 4), count(good, 1ull << 61),
      count(good, 2), good.substr(0, 7), "", items_image({it[0], it[1], {it[1].first, it[2].second}}),
      items_image({it[0], it[2], it[1]}), items_image({{it[1].first + "a", 0}, it[1]}),
      fgood.substr(0, fgood.size() - 1), fgood + std::string(1, '\0'), count(fgood, 6),
      items_image({fi[0], fi[1], fi[2], fi[2], fi[4]}), items_image({fi[0], fi[1], fi[3], fi[2], fi[4]}), klen_off};
  for (size_t k = 0; k < bad.size(); ++k)
    for (uint32_t at = 0; at < 3; ++at) {  // the refused table first, in the middle, last
      Batch b;
      for (uint32_t j = 0; j < 3; ++j) {
        const bool fx = k >= 10;
        b.add_table(data_image(fx ? f : t), j == at ? bad[k] : (j % 2 ? fgood : good));
        (void)fx;
      }
      b.set_keys({"k", t[3].first});
      check(b, "refused index", at);
      CHECK(!ref_map(bad[k]).ok, "refused index %zu: the model refuses it too", k);
    }
  // two refused tables: the first is named; spans past their arenas
  Batch b;
  for (int j = 0; j < 4; ++j) b.add_table(data_image(t), j == 1 || j == 3 ? bad[0] : good);
  b.set_keys({t[3].first});
  check(b, "two refused", 1);
  Batch c;
  for (int j = 0; j < 3; ++j) c.add_table(data_image(t), good);
  c.set_keys({t[3].first, t[4].first, ""});
  std::vector<lsmck_sstable_span> s = c.spans;
  s[2].data_len += 1;
  check(c, "data span past the arena", 2, ~0ull, &s);
  s = c.spans, s[1].index_off = c.index.size() + 1, s[1].index_len = 0;
  check(c, "index span past the arena", 1, ~0ull, &s);
  s = c.spans, s[0].data_off = ~0ull - 3;
  check(c, "data span wraps", 0, ~0ull, &s);
  s = c.spans, s[2].index_len = ~0ull;
  check(c, "index span wraps", 2, ~0ull, &s);
  // queries
  std::vector<lsmck_get_query> q = c.q;
  q[1].klen += 1000;
  check(c, "query key past qkeys", ~0ull, 1, nullptr, &q);
  q = c.q, q[0].key_off = ~0ull;
  check(c, "query offset wraps", ~0ull, 0, nullptr, &q);
  q = c.q, q[2].reserved = 1;
  check(c, "reserved", ~0ull, 2, nullptr, &q);
  q = c.q, q[2].key_off = ~0ull;  // (an empty key's offset is not looked at)
  check(c, "empty key anywhere", ~0ull, ~0ull, nullptr, &q);
  q = c.q, q[1].reserved = 7, q[2].reserved = 7;
  s = c.spans, s[2].data_len += 1;
  check(c, "tables before queries", 2, ~0ull, &s, &q);
}

static void test_overlapping_index_spans() {
  // every table reads one index image: more items than index_bytes / 16 + ntab slots
  Entries e;
  for (int i = 0; i < 40; ++i) e.push_back({std::string(1, (char)('A' + i)), "v"});
  Batch b;
  b.add_table(data_image(e), items_image(items_of(e, 1)));
  std::vector<lsmck_sstable_span> s(30, b.spans[0]);
  b.tables.assign(30, b.tables[0]);
  b.set_keys(queries_for({e}));
  const Out O = check(b, "overlapping index spans", ~0ull, ~0ull, &s);
  CHECK(O.regrow, "overlapping index spans: the passes ran twice");
}

static void test_no_tables_no_queries() {
  Batch b;
  b.set_keys({"a", ""});
  const Out O = check(b, "no tables");
  CHECK(O.res.size() == 2 && O.res[0].table == LSMCK_GET_NONE && O.res[0].val_off == 0 && O.res[0].vlen == 0, "no tables");
  Batch c;
  c.add_table("", items_image({}));
  c.set_keys({});
  check(c, "no queries");
}

int main() {
  static_assert(sizeof(lsmck_get_query) == 16 && sizeof(lsmck_get_result) == 16, "the ABI's structs");
  test_sizes();
  test_ties();
  test_doctored();
  test_cuts();
  test_refusals();
  test_overlapping_index_spans();
  test_no_tables_no_queries();
  if (fails) {
    printf("%d failure(s)\n", fails);
    return 1;
  }
  printf("sstget ok\n");
  return 0;
}
