// Host model of the opened table set (csrc/lsmck_tableset.h): the steps the
// kernels of lsmck_tableset.hip run -- the index pass's item offsets, order
// keys and positions (the serial parse; the in-place proof of an index of one
// key length is tests/native/test_sstget.cpp's), ts::fences per table at open,
// then per get every (query, table) pair behind ts::fenced with the winner's
// minimum, and resolve -- in the kernels' order and with the pairs in both
// orders, compared with get::table_get WITHOUT fences and with a model that
// parses the index into a std::map and runs SsTable::get's two branches as
// loops over bytes.  Every fenced pair must be None under both.  Built with
// -fsanitize=address,undefined: the data, index and query arenas are
// exact-size heap blocks with tables flush against both ends, so a fence walk
// or a tie compare that reads outside an image is caught.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "lsmck_tableset.h"

using namespace lsmck;
typedef std::vector<std::pair<std::string, std::string>> Entries;
typedef std::vector<std::pair<std::string, uint64_t>> Items;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
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
typedef std::map<std::string, uint64_t> RefMap;
static RefMap ref_map(const std::string& x) {  // (every index here is a map image)
  RefMap m;
  const uint64_t count = rd(x, 0, 8);
  uint64_t at = 8;
  for (uint64_t j = 0; j < count; ++j) {
    const uint64_t kl = rd(x, at, 8);
    m[x.substr(at + 8, kl)] = rd(x, at + 8 + kl, 8);
    at += 16 + kl;
  }
  CHECK(at == x.size() && m.size() == count, "the model's index images are maps");
  return m;
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
static bool ref_get(const std::string& d, const RefMap& m, const std::string& key, uint64_t* vpos, uint64_t* vlen) {
  RefRec r;
  auto hit = m.find(key);
  if (hit != m.end()) {
    if (!ref_read(d, hit->second, &r)) return false;
    *vpos = r.kpos + r.klen, *vlen = r.vlen;
    return true;
  }
  auto lb = m.lower_bound(key);
  uint64_t pos = lb == m.begin() ? 0 : std::prev(lb)->second;
  const uint64_t end = lb == m.end() ? d.size() : lb->second;
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
// the fences, restated over strings: the walk's keys, its end within the cap
static bool ref_walk(const std::string& d, uint64_t start, uint64_t end, uint32_t cap, std::vector<std::string>* seen) {
  RefRec r;
  uint64_t pos = start;
  while (ref_read(d, pos, &r)) {
    if (seen->size() == cap) return false;
    seen->push_back(d.substr(r.kpos, r.klen));
    pos += r.size;
    if (pos >= end) break;
  }
  return true;
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

// the opened set: what lsmck_tableset_open leaves
struct Set {
  std::vector<uint64_t> first, ioff, ipos;
  std::vector<mrg::OKey> iok;
  std::vector<ts::Fence> fence;
  uint64_t low = 0, high = 0;
};
static get::Table table_of(const Set& S, const Batch& b, const uint8_t* data, const uint8_t* index, uint64_t t) {
  get::Table T;
  T.img = data + b.spans[t].data_off, T.dlen = b.spans[t].data_len, T.idx = index + b.spans[t].index_off;
  T.ok = S.iok.data() + S.first[t], T.ioff = S.ioff.data() + S.first[t], T.ipos = S.ipos.data() + S.first[t];
  T.nitems = S.first[t + 1] - S.first[t];
  return T;
}
static Set open_set(const Batch& b, const uint8_t* data, const uint8_t* index, uint32_t cap) {
  const uint64_t ntab = b.spans.size();
  Set S;
  S.first.assign(ntab + 1, 0);
  for (uint64_t t = 0; t < ntab; ++t) {
    const uint64_t c = get::index_parse(index + b.spans[t].index_off, b.spans[t].index_len, nullptr, 0);
    CHECK(c != get::kNo, "every index here parses");
    S.first[t + 1] = S.first[t] + c;
  }
  const uint64_t total = S.first[ntab];
  S.ioff.resize(total + 1), S.ipos.resize(total + 1), S.iok.resize(total + 1);
  for (uint64_t t = 0; t < ntab; ++t) {
    const uint8_t* idx = index + b.spans[t].index_off;
    const uint64_t k = S.first[t + 1] - S.first[t];
    if (k) CHECK(get::index_parse(idx, b.spans[t].index_len, S.ioff.data() + S.first[t], k) == k, "the fill");
    for (uint64_t sl = S.first[t]; sl < S.first[t + 1]; ++sl) {
      S.iok[sl] = get::item_okey(idx, S.ioff[sl]);
      S.ipos[sl] = get::item_pos(idx, S.ioff[sl]);
      if (sl > S.first[t]) CHECK(get::item_less(idx, S.ioff[sl - 1], S.ioff[sl]), "the items' order");
    }
  }
  // ts_fences: a lane per table
  S.fence.resize(ntab);
  for (uint64_t t = 0; t < ntab; ++t) {
    S.fence[t] = ts::fences(table_of(S, b, data, index, t), cap);
    S.low += (S.fence[t].valid & ts::kLow) != 0, S.high += (S.fence[t].valid & ts::kHigh) != 0;
  }
  return S;
}
static std::string fkey_str(const ts::FKey& f) { return std::string((const char*)f.p, (size_t)f.klen); }

struct Out {
  std::vector<lsmck_get_result> res;
  uint64_t fenced = 0, probed = 0, skipped = 0;
};
// the get: ts_probe over the pairs in one order or the other, then resolve
static Out get_batch(const Set& S, const Batch& b, const uint8_t* data, const uint8_t* index, const uint8_t* qkeys,
                     bool reversed, bool use_fences) {
  const uint64_t ntab = b.spans.size(), n = b.q.size();
  Out O;
  std::vector<mrg::OKey> qok(n);
  std::vector<uint32_t> win(n, get::kNoTable);
  for (uint64_t i = 0; i < n; ++i) qok[i] = get::key_of(qkeys, b.q[i].key_off, b.q[i].klen).ok;
  auto key = [&](uint64_t i) {
    get::Key k;
    k.p = b.q[i].klen ? qkeys + b.q[i].key_off : qkeys;
    k.ok = qok[i];
    return k;
  };
  const uint64_t total = n * ntab;
  for (uint64_t x = 0; x < total; ++x) {
    const uint64_t w = reversed ? total - 1 - x : x, t = w / n, i = w - t * n;
    if (use_fences && ts::fenced(S.fence[t], key(i))) {
      ++O.fenced;
      continue;
    }
    if (t > win[i]) {
      ++O.skipped;
      continue;
    }
    uint64_t vpos;
    uint32_t vlen;
    bool walked;
    if (get::table_get(table_of(S, b, data, index, t), key(i), &vpos, &vlen, &walked)) win[i] = std::min<uint32_t>(win[i], (uint32_t)t);
    ++O.probed;
  }
  O.res.resize(n);
  for (uint64_t i = 0; i < n; ++i) {
    lsmck_get_result r = get::result_none();
    if (win[i] != get::kNoTable) {
      const get::Table T = table_of(S, b, data, index, win[i]);
      uint64_t vpos;
      uint32_t vlen;
      const bool some = get::table_get(T, key(i), &vpos, &vlen, nullptr);
      CHECK(some, "resolve finds what probe found (query %llu)", (unsigned long long)i);
      if (some) r = get::result_of(T.img, b.spans[win[i]].data_off, vpos, vlen, win[i]);
    }
    O.res[i] = r;
  }
  return O;
}

// the batch through exact-size blocks at one cap: fences against their
// restatement, every fenced pair None, both pair orders, fences on and off,
// the std::map model
struct Counts {
  uint64_t low, high, fenced;
};
static Counts check(const Batch& b, const char* what, uint32_t cap) {
  Heap D(b.data), X(b.index), K(b.qkeys);
  const Set S = open_set(b, D.p, X.p, cap);
  const uint64_t ntab = b.spans.size(), n = b.q.size();
  std::vector<RefMap> maps;
  for (uint64_t t = 0; t < ntab; ++t) maps.push_back(ref_map(b.tables[t].second));
  uint64_t want_fenced = 0;
  for (uint64_t t = 0; t < ntab; ++t) {
    // the fence against its restatement over strings
    const std::string& d = b.tables[t].first;
    const ts::Fence& F = S.fence[t];
    bool low = false, high = false;
    std::string lo, hi;
    if (!maps[t].empty()) {
      std::vector<std::string> seen;
      lo = maps[t].begin()->first;
      low = ref_walk(d, 0, maps[t].begin()->second, cap, &seen);
      for (auto& k : seen) low = low && !(k < lo);
      seen.clear();
      hi = maps[t].rbegin()->first;
      high = ref_walk(d, maps[t].rbegin()->second, d.size(), cap, &seen);
      for (auto& k : seen) hi = std::max(hi, k);
    }
    CHECK(((F.valid & ts::kLow) != 0) == low && ((F.valid & ts::kHigh) != 0) == high, "%s: table %llu cap %u: valid %u, want %d %d",
          what, (unsigned long long)t, cap, F.valid, low, high);
    if (low) CHECK(fkey_str(F.lo) == lo, "%s: table %llu: the low fence is key_0", what, (unsigned long long)t);
    if (high) CHECK(fkey_str(F.hi) == hi, "%s: table %llu: the high fence is the tail's maximum", what, (unsigned long long)t);
    // every pair: fenced iff the restatement says so, and then None both ways
    for (uint64_t i = 0; i < n; ++i) {
      const std::string& k = b.keys[i];
      const bool want = (low && k < lo) || (high && hi < k);
      get::Key key = get::key_of(K.p, b.q[i].key_off, b.q[i].klen);
      const bool got = ts::fenced(F, key);
      CHECK(got == want, "%s: table %llu query %llu cap %u: fenced %d, want %d", what, (unsigned long long)t,
            (unsigned long long)i, cap, got, want);
      want_fenced += want;
      if (got) {
        uint64_t vpos, vl64;
        uint32_t vlen;
        CHECK(!ref_get(d, maps[t], k, &vpos, &vl64), "%s: table %llu query %llu: a fenced pair is None in the model", what,
              (unsigned long long)t, (unsigned long long)i);
        CHECK(!get::table_get(table_of(S, b, D.p, X.p, t), key, &vpos, &vlen, nullptr),
              "%s: table %llu query %llu: a fenced pair is None in table_get", what, (unsigned long long)t, (unsigned long long)i);
      }
    }
  }
  const Out O = get_batch(S, b, D.p, X.p, K.p, false, true), R = get_batch(S, b, D.p, X.p, K.p, true, true);
  const Out P = get_batch(S, b, D.p, X.p, K.p, false, false);
  CHECK(O.fenced == want_fenced && R.fenced == want_fenced, "%s: the fenced count does not depend on the pairs' order", what);
  CHECK(O.fenced + O.probed + O.skipped == n * ntab, "%s: every pair is fenced, skipped or looked up", what);
  for (const Out* other : {&R, &P})
    CHECK(other->res.size() == n && (!n || !memcmp(other->res.data(), O.res.data(), 16 * n)),
          "%s: neither the pairs' order nor the fences change a result", what);
  for (uint64_t i = 0; i < n; ++i) {
    lsmck_get_result want = get::result_none();
    for (uint64_t t = 0; t < ntab; ++t) {
      uint64_t vpos, vlen;
      const std::string& d = b.tables[t].first;
      if (!ref_get(d, maps[t], b.keys[i], &vpos, &vlen)) continue;
      want.val_off = b.spans[t].data_off + vpos, want.vlen = (uint32_t)vlen, want.table = (uint32_t)t;
      if (vlen == 1 && d[vpos] == 0) want.val_off |= LSMCK_GET_TOMBSTONE;
      break;
    }
    const lsmck_get_result g = O.res[i];
    CHECK(g.val_off == want.val_off && g.vlen == want.vlen && g.table == want.table,
          "%s: query %llu: (%llx, %u, %u), want (%llx, %u, %u)", what, (unsigned long long)i, (unsigned long long)g.val_off,
          g.vlen, g.table, (unsigned long long)want.val_off, want.vlen, want.table);
  }
  return {S.low, S.high, O.fenced};
}
static void check_caps(const Batch& b, const char* what) {
  Counts prev = {0, 0, 0};
  for (uint32_t cap : {1u, 4u, 256u}) {
    const Counts c = check(b, what, cap);
    CHECK(c.low >= prev.low && c.high >= prev.high && c.fenced >= prev.fenced, "%s: a larger cap loses no fence", what);
    prev = c;
  }
}

// ---- cases ------------------------------------------------------------------------
static Entries make_table(uint32_t m, uint32_t seed, uint32_t base) {
  Entries t;
  char buf[64];
  for (uint32_t i = 0; i < m; ++i) {
    snprintf(buf, sizeof buf, "k%07u", base + i * 3);
    std::string k = std::string(buf) + std::string((i * 5 + seed) % 11, 'x'), v;
    if ((i + seed) % 11 == 3) v = "";
    else if ((i + seed) % 13 == 5) v = std::string(1, '\0');  // a tombstone
    else v = std::string((i * 7 + seed) % 19 + 1, (char)('0' + i % 10));
    t.push_back({k, v});
  }
  std::sort(t.begin(), t.end());
  return t;
}
static void around(std::vector<std::string>* ks, const std::string& k) {
  ks->push_back(k);
  ks->push_back(k + std::string(1, '\0'));
  if (k.empty()) return;
  ks->push_back(k.substr(0, k.size() - 1));
  std::string lo = k;
  if ((uint8_t)lo.back() == 0) lo.pop_back();
  else lo.back() = (char)((uint8_t)lo.back() - 1), lo += "\xff\xff";
  ks->push_back(lo);
}
static std::vector<std::string> queries_for(const std::vector<Entries>& tabs) {
  std::vector<std::string> ks = {"", std::string(19, (char)0xff), "k", "a"};
  for (auto& t : tabs)
    for (size_t i = 0; i < t.size(); ++i)
      if (i < 3 || i + 3 >= t.size() || i % 50 < 2 || below(8) == 0) around(&ks, t[i].first);
  return ks;
}

static void test_random() {
  // overlapping and disjoint ranges, sizes around the index step, sound tables and doctored items
  for (int round = 0; round < 24; ++round) {
    Batch b;
    b.front(below(16));
    std::vector<Entries> tabs;
    const uint32_t ntab = 2 + below(6);
    for (uint32_t j = 0; j < ntab; ++j) {
      const uint32_t sizes[] = {0, 1, 2, 99, 100, 101, 199, 201, 260};
      const Entries e = make_table(sizes[below(9)], round + j, round % 2 ? j * 1000 : below(300));
      tabs.push_back(e);
      Items items = items_of(e, 100);
      std::vector<uint64_t> pos;
      const std::string d = data_image(e, &pos);
      if (!items.empty() && !e.empty()) switch (below(8)) {
          case 0: items[below(items.size())].second = pos[below(e.size())]; break;      // another record's position
          case 1: items.back().second = d.size() - below(12); break;                    // at the end, or no header fits
          case 2: items[below(items.size())].second = pos[below(e.size())] + 1 + below(7); break;  // mid-record
          case 3: items.erase(items.begin()); break;                                    // the first item missing
          case 4: items[below(items.size())].second = rnd() | (1ull << 63); break;      // far past the end
          case 5: items[0].second = pos[std::min<size_t>(e.size() - 1, 1 + below(5))]; break;  // pos_0 > 0
          default: break;
        }
      const size_t cut = below(4) == 0 ? below(20) : 0;  // a tail ending in a cut record
      b.add_table(d.substr(0, d.size() - std::min(cut, d.size())), items_image(items));
    }
    b.set_keys(queries_for(tabs));
    check_caps(b, "random");
  }
}

static void test_doctored() {
  Entries e;
  char buf[32];
  for (int i = 0; i < 250; ++i) snprintf(buf, sizeof buf, "d%04d", i), e.push_back({buf, "val" + std::to_string(i)});
  std::vector<uint64_t> pos;
  const std::string d = data_image(e, &pos);
  auto k = [&](int i) { return e[i].first; };
  Batch b;
  b.front(5);
  std::vector<std::string> ks = {"", std::string(20, (char)0xff)};
  // the first item missing: the head's keys lie below key_0
  b.add_table(d, items_image({{k(100), pos[100]}, {k(200), pos[200]}}));
  // a record at 0 below key_0 while pos_0 = 0
  Entries low0 = e;
  low0[0] = {"a-low", "found-below-key0"};
  std::vector<uint64_t> lp;
  const std::string ld = data_image(low0, &lp);
  b.add_table(ld, items_image({{k(0), 0}, {k(100), lp[100]}, {k(200), lp[200]}}));
  // an unsorted tail whose maximum is not its last record
  Entries tail(e.begin(), e.begin() + 200);
  for (auto& x : Entries{{"d0200", "x"}, {"zz-max", "top"}, {"d0100a", "back"}, {"m-last", "end"}}) tail.push_back(x);
  std::vector<uint64_t> tp;
  const std::string td = data_image(tail, &tp);
  b.add_table(td, items_image({{k(0), 0}, {k(100), tp[100]}, {k(200), tp[200]}}));
  // cut tails
  b.add_table(d.substr(0, d.size() - 2), items_image({{k(0), 0}, {k(200), pos[200]}}));
  b.add_table(d.substr(0, pos[249] + 5), items_image({{k(0), 0}, {k(200), pos[200]}}));
  // pos_{m-1} at and past L
  b.add_table(d, items_image({{k(0), 0}, {k(200), d.size()}}));
  b.add_table(d, items_image({{k(0), 0}, {k(200), (1ull << 63) + 9}}));
  b.add_table(d, items_image({{k(0), 0}, {k(200), ~0ull}}));
  b.add_table(d, items_image({{k(0), 0}, {k(100), pos[100]}, {k(200), pos[5]}}));
  // heads and tails around the caps
  Entries lng, four;
  for (int i = 0; i < 20; ++i) snprintf(buf, sizeof buf, "h%02d", i), lng.push_back({buf, "v"});
  for (int i = 0; i < 8; ++i) snprintf(buf, sizeof buf, "f%02d", i), four.push_back({buf, "w"});
  std::vector<uint64_t> gp, fp;
  const std::string gd = data_image(lng, &gp), fd = data_image(four, &fp);
  b.add_table(gd, items_image({{"h00", gp[7]}, {"h11", gp[11]}}));
  b.add_table(fd, items_image({{"f00", fp[4]}, {"f04", fp[4]}}));
  // m == 0, with and without data
  b.add_table(data_image(Entries(e.begin(), e.begin() + 5)), items_image({}));
  b.add_table("", items_image({}));
  // ties past 8 bytes, proper prefixes, the empty key
  Entries t;
  for (const char* s : {"aaaa", "aaab", "bbbbbbbbbbbbbbbb", "bbbbbbbbbbbbbbbc"}) t.push_back({std::string("TIEDKEY-") + s, "v"});
  std::vector<uint64_t> ip;
  const std::string tied = data_image(t, &ip);
  b.add_table(tied, items_image({{t[0].first, 0}, {t[2].first, ip[2]}}));
  b.add_table(data_image({{"prefix-89", "1"}, {"prefix-89abc", "2"}}), items_image({{"prefix-89", 0}}));
  b.add_table(data_image({{"", "empty-key"}, {"a", std::string(1, '\0')}, {"b", ""}}), items_image({{"", 0}}));
  b.add_table(data_image({{"k1", "1"}, {"", "late-empty"}}), items_image({{"k1", 0}}));
  for (const std::string& key :
       {k(0), k(50), k(99), k(100), k(200), k(201), k(248), k(249), k(5), std::string("a-low"), std::string("zz-max"),
        std::string("m-last"), std::string("d0100a"), std::string("h00"), std::string("h06"), std::string("h07"), std::string("h11"),
        std::string("h19"), std::string("f00"), std::string("f03"), std::string("f04"), std::string("f07"), t[0].first, t[1].first,
        t[3].first, std::string("TIEDKEY-"), std::string("TIEDKEY-bbbbbbbb"), std::string("prefix-89"), std::string("prefix-89abc"),
        std::string("k1"), std::string("a"), std::string("b")})
    around(&ks, key);
  b.set_keys(ks);
  check_caps(b, "doctored");
  const Counts c1 = check(b, "doctored", 1), c4 = check(b, "doctored", 4), c256 = check(b, "doctored", 256);
  CHECK(c1.high < c4.high && c4.high < c256.high && c1.low < c256.low, "doctored: the caps 1, 4 and 256 give different fences");
}

static void test_wide() {
  // 40 tables of 12 records over disjoint ranges: all but a key's own table are fenced
  Batch b;
  std::vector<std::string> ks;
  char buf[32];
  for (int t = 0; t < 40; ++t) {
    Entries e;
    for (int i = 0; i < 12; ++i) snprintf(buf, sizeof buf, "w%04d-%04d", t, 2 * i), e.push_back({buf, "v" + std::to_string(i)});
    b.add_table(data_image(e), items_image(items_of(e, 100)));
  }
  for (int i = 0; i < 200; ++i) snprintf(buf, sizeof buf, "w%04d-%04d", (int)below(40), (int)below(23)), ks.push_back(buf);
  b.set_keys(ks);
  const Counts c = check(b, "wide", 256);
  CHECK(c.low == 40 && c.high == 40 && c.fenced == 39 * 200, "wide: 39 of 40 tables are fenced for every key");
}

static void test_empty() {
  Batch b;
  b.set_keys({"a", ""});
  check(b, "no tables", 256);
  Batch c;
  c.add_table("", items_image({}));
  c.set_keys({});
  check(c, "no queries", 256);
}

int main() {
  static_assert(sizeof(ts::Fence) == 80, "the fence record");
  test_random();
  test_doctored();
  test_wide();
  test_empty();
  if (fails) {
    printf("%d failure(s)\n", fails);
    return 1;
  }
  printf("tableset ok\n");
  return 0;
}
