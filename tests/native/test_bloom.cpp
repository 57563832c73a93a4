// Host model of the opened table set's bloom filters (csrc/lsmck_bloom.h): the
// steps the kernels of lsmck_tableset.hip run when a set is opened with
// "bloom_bits" -- a lane per (table, interval) found by blm::interval_table,
// pass 1 (blm::count) into per-table key counts and the over-the-cap marks,
// the sizes' scan, pass 2 (blm::fill) into a zeroed, exact-size filter buffer
// -- and per get the queries' hashes once, then every (query, table) pair
// behind ts::fenced and blm::drops with the winner's minimum, and resolve: in
// the kernels' order and with the pairs in both orders, at the caps 1, 4 and
// 256 and 4, 12 and 64 bits per key, compared with the same get WITHOUT
// filters, with get::table_get and with a model that parses the index into a
// std::map and runs SsTable::get's two branches as loops over bytes.  Every
// pair a filter drops must be None under both; the key counts and the tables
// with a filter are restated over strings.  The hash's known answers are the
// numbers of tests/test_bloom_cases.py.  Built with
// -fsanitize=address,undefined: the arenas and the filter buffer are
// exact-size heap blocks.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "lsmck_bloom.h"
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

// ---- the filters: what lsmck_tableset_open leaves with "bloom_bits" > 0 ----------------
struct Bloom {
  std::vector<blm::Desc> desc;
  uint32_t* filt = nullptr;  // an exact-size block
  uint64_t blocks = 0, tables = 0, keys = 0;
  std::vector<uint64_t> nkeys;
  ~Bloom() { free(filt); }
};
static void open_bloom(Bloom* B, const Set& S, const Batch& b, const uint8_t* data, const uint8_t* index, uint32_t cap,
                       uint32_t bits) {
  const uint64_t ntab = b.spans.size(), lanes = S.first[ntab] + ntab;
  std::vector<uint32_t> over(ntab, 0);
  B->nkeys.assign(ntab, 0);
  // ts_bloom_count: a lane per (table, interval)
  std::vector<uint64_t> seen_lanes(ntab, 0);
  for (uint64_t g = 0; g < lanes; ++g) {
    const uint64_t t = blm::interval_table(S.first.data(), ntab, g), j = g - blm::interval_first(S.first.data(), t);
    CHECK(t < ntab && j <= S.first[t + 1] - S.first[t], "lane %llu: table %llu interval %llu", (unsigned long long)g,
          (unsigned long long)t, (unsigned long long)j);
    ++seen_lanes[t];
    uint64_t n = 0;
    if (!blm::count(table_of(S, b, data, index, t), j, cap, &n)) over[t] = 1;
    B->nkeys[t] += n;
  }
  for (uint64_t t = 0; t < ntab; ++t)
    CHECK(seen_lanes[t] == S.first[t + 1] - S.first[t] + 1, "table %llu has m + 1 lanes", (unsigned long long)t);
  // ts_bloom_size
  B->desc.resize(ntab);
  for (uint64_t t = 0; t < ntab; ++t) {
    const uint32_t nb = over[t] ? 0u : blm::nblocks_of(B->nkeys[t], bits);
    B->desc[t].first = nb ? B->blocks : 0, B->desc[t].nblocks = nb, B->desc[t].valid = nb ? 1u : 0u;
    B->blocks += nb;
    if (nb) ++B->tables, B->keys += B->nkeys[t];
  }
  B->filt = (uint32_t*)calloc(B->blocks ? B->blocks * blm::kWords : 1, 4);
  // ts_bloom_fill, the lanes in the other order
  for (uint64_t g = lanes; g-- > 0;) {
    const uint64_t t = blm::interval_table(S.first.data(), ntab, g), j = g - blm::interval_first(S.first.data(), t);
    if (B->desc[t].valid) blm::fill(table_of(S, b, data, index, t), j, cap, B->filt, B->desc[t]);
  }
}

struct Out {
  std::vector<lsmck_get_result> res;
  uint64_t fenced = 0, bloomed = 0, probed = 0, skipped = 0;
};
// the get: ts_hash, ts_probe<true> (or <false>: B == nullptr) over the pairs in one order or the other, then resolve
static Out get_batch(const Set& S, const Bloom* B, const Batch& b, const uint8_t* data, const uint8_t* index,
                     const uint8_t* qkeys, bool reversed) {
  const uint64_t ntab = b.spans.size(), n = b.q.size();
  Out O;
  std::vector<mrg::OKey> qok(n);
  std::vector<uint64_t> qh(n);
  std::vector<uint32_t> win(n, get::kNoTable);
  for (uint64_t i = 0; i < n; ++i) {
    qok[i] = get::key_of(qkeys, b.q[i].key_off, b.q[i].klen).ok;
    qh[i] = blm::hash(b.q[i].klen ? qkeys + b.q[i].key_off : qkeys, b.q[i].klen);
  }
  auto key = [&](uint64_t i) {
    get::Key k;
    k.p = b.q[i].klen ? qkeys + b.q[i].key_off : qkeys;
    k.ok = qok[i];
    return k;
  };
  const uint64_t total = n * ntab;
  for (uint64_t x = 0; x < total; ++x) {
    const uint64_t w = reversed ? total - 1 - x : x, t = w / n, i = w - t * n;
    if (ts::fenced(S.fence[t], key(i))) {
      ++O.fenced;
      continue;
    }
    if (B && blm::drops(B->filt, B->desc[t], qh[i])) {
      ++O.bloomed;
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

struct Counts {
  uint64_t tables, keys, bloomed;
};
static Counts check(const Batch& b, const char* what, uint32_t cap, uint32_t bits) {
  Heap D(b.data), X(b.index), K(b.qkeys);
  const Set S = open_set(b, D.p, X.p, cap);
  Bloom B;
  open_bloom(&B, S, b, D.p, X.p, cap, bits);
  const uint64_t ntab = b.spans.size(), n = b.q.size();
  std::vector<RefMap> maps;
  for (uint64_t t = 0; t < ntab; ++t) maps.push_back(ref_map(b.tables[t].second));
  uint64_t want_tables = 0, want_keys = 0;
  for (uint64_t t = 0; t < ntab; ++t) {
    // the key set restated over strings: the item keys and every walk's records
    const std::string& d = b.tables[t].first;
    std::vector<std::string> keys;
    std::vector<uint64_t> starts = {0}, ends;
    for (auto& it : maps[t]) keys.push_back(it.first), starts.push_back(it.second), ends.push_back(it.second);
    ends.push_back(d.size());
    bool ok = true;
    for (size_t j = 0; j < starts.size(); ++j) {
      std::vector<std::string> seen;
      ok = ref_walk(d, starts[j], ends[j], cap, &seen) && ok;
      keys.insert(keys.end(), seen.begin(), seen.end());
    }
    const blm::Desc& F = B.desc[t];
    CHECK((F.valid != 0) == ok, "%s: table %llu cap %u: valid %u, want %d", what, (unsigned long long)t, cap, F.valid, ok);
    CHECK(B.nkeys[t] == keys.size() || !ok, "%s: table %llu cap %u: %llu keys, want %llu", what, (unsigned long long)t, cap,
          (unsigned long long)B.nkeys[t], (unsigned long long)keys.size());
    if (!ok) continue;
    ++want_tables, want_keys += keys.size();
    const uint64_t nb = std::max<uint64_t>(1, (keys.size() * bits + 255) / 256);
    CHECK(F.nblocks == nb, "%s: table %llu: %u blocks, want %llu", what, (unsigned long long)t, F.nblocks, (unsigned long long)nb);
    // no key of the set is dropped
    for (auto& k : keys)
      CHECK(!blm::drops(B.filt, F, blm::hash((const uint8_t*)k.data(), k.size())), "%s: table %llu drops a key of its own", what,
            (unsigned long long)t);
    // a dropped pair is None both ways
    for (uint64_t i = 0; i < n; ++i) {
      const get::Key key = get::key_of(K.p, b.q[i].key_off, b.q[i].klen);
      if (!blm::drops(B.filt, F, blm::hash(key.p, b.q[i].klen))) continue;
      uint64_t vpos, vl64;
      uint32_t vlen;
      CHECK(!ref_get(d, maps[t], b.keys[i], &vpos, &vl64), "%s: table %llu query %llu: a dropped pair is None in the model", what,
            (unsigned long long)t, (unsigned long long)i);
      CHECK(!get::table_get(table_of(S, b, D.p, X.p, t), key, &vpos, &vlen, nullptr),
            "%s: table %llu query %llu: a dropped pair is None in table_get", what, (unsigned long long)t, (unsigned long long)i);
    }
  }
  CHECK(B.tables == want_tables && B.keys == want_keys, "%s: cap %u: %llu tables with %llu keys, want %llu with %llu", what, cap,
        (unsigned long long)B.tables, (unsigned long long)B.keys, (unsigned long long)want_tables, (unsigned long long)want_keys);
  const Out O = get_batch(S, &B, b, D.p, X.p, K.p, false), R = get_batch(S, &B, b, D.p, X.p, K.p, true);
  const Out P = get_batch(S, nullptr, b, D.p, X.p, K.p, false);
  CHECK(O.bloomed == R.bloomed && O.fenced == R.fenced && O.fenced == P.fenced,
        "%s: the counts do not depend on the pairs' order, the fenced count not on the filters", what);
  CHECK(O.fenced + O.bloomed + O.probed + O.skipped == n * ntab, "%s: every pair is fenced, dropped, skipped or looked up", what);
  for (const Out* other : {&R, &P})
    CHECK(other->res.size() == n && (!n || !memcmp(other->res.data(), O.res.data(), 16 * n)),
          "%s: neither the pairs' order nor the filters change a result", what);
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
  return {B.tables, B.keys, O.bloomed};
}
static uint64_t total_bloomed = 0;
static void check_all(const Batch& b, const char* what) {
  for (uint32_t bits : {4u, 12u, 64u}) {
    Counts prev = {0, 0, 0};
    for (uint32_t cap : {1u, 4u, 256u}) {
      const Counts c = check(b, what, cap, bits);
      CHECK(c.tables >= prev.tables, "%s: a larger cap loses no filter", what);
      prev = c;
      total_bloomed += c.bloomed;
    }
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
  for (int round = 0; round < 12; ++round) {
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
    check_all(b, "random");
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
  check_all(b, "doctored");
  const Counts c1 = check(b, "doctored", 1, 12), c4 = check(b, "doctored", 4, 12), c256 = check(b, "doctored", 256, 12);
  CHECK(c1.tables < c4.tables && c4.tables < c256.tables, "doctored: the caps 1, 4 and 256 give different filters");
}

static void test_interleaved() {
  // 4 tables whose 16-byte keys interleave and tie past 8 bytes: nothing is fenced, the absent keys are dropped
  Batch b;
  std::vector<std::string> ks;
  auto key16 = [](uint64_t x) {
    std::string k(8, '\0');
    for (int s = 56; s >= 0; s -= 8) k.push_back((char)(x >> s));
    return k;
  };
  for (uint64_t t = 0; t < 4; ++t) {
    Entries e;
    for (uint64_t i = 0; i < 250; ++i) e.push_back({key16(8 * i + t), "v" + std::to_string(i)});
    b.add_table(data_image(e), items_image(items_of(e, 100)));
  }
  for (int i = 0; i < 400; ++i) ks.push_back(key16(8 * (1 + below(248)) + below(4) + (i % 2 ? 4 : 0)));
  b.set_keys(ks);
  const Counts c = check(b, "interleaved", 256, 12);
  CHECK(c.tables == 4 && c.keys == 4 * (250 + 3 + 1), "interleaved: four filters over 254 keys each");
  CHECK(c.bloomed >= 9 * (4 * 200 + 3 * 200) / 10, "interleaved: %llu pairs dropped", (unsigned long long)c.bloomed);
}

static void test_lengths() {
  // a key of every length 0..24: the hash's tail word and its length term, at every alignment of the key
  const uint64_t known[25] = {
      0x0000000000000000ull, 0x9E0160293A33AAF7ull, 0xEBD1BD6E1374CB0Dull, 0x4B6FB9192CB85E54ull, 0x958C922B50D90CE3ull,
      0x7DE43CC28CDD9AB5ull, 0xA02A6AB0FA9EC8D9ull, 0x06F04AC25E0D20B3ull, 0x2D26208944ED5837ull, 0x0D1740B607B11A4Cull,
      0x2AE626ADC758D79Bull, 0xEFF24E8B8F4D2C15ull, 0x9BDC06C0036828C9ull, 0x9979B164C771CBDAull, 0xCB52A57C251065F5ull,
      0x46ED73D1CD8BD7DDull, 0xA9096F9E18B7AB22ull, 0x4CD22D92EB2B4D2Bull, 0x3348C676A1B33B7Cull, 0xE0DF011DDEF51775ull,
      0x4699E22D06EF3B92ull, 0xDDC87583F442E630ull, 0x3D288599E95F6FFDull, 0xB71DE39302D90497ull, 0xC45E1CC1E2E574C0ull};
  for (uint32_t n = 0; n <= 24; ++n)
    for (uint32_t shift = 0; shift < 4; ++shift) {
      std::string s(shift, (char)0xEE);
      for (uint32_t j = 1; j <= n; ++j) s.push_back((char)j);
      Heap H(s);  // the key ends flush with the block
      const uint64_t h = blm::hash(H.p + shift, n);
      CHECK(h == known[n], "hash of length %u at shift %u: %016llx, want %016llx", n, shift, (unsigned long long)h,
            (unsigned long long)known[n]);
    }
  CHECK(blm::mix(1) == 0x5692161D100B05E5ull, "splitmix64's finaliser");
  CHECK(blm::nblocks_of(0, 12) == 1 && blm::nblocks_of(64, 4) == 1 && blm::nblocks_of(65, 4) == 2 && blm::nblocks_of(5, 64) == 2,
        "the blocks of a few keys");
  CHECK(blm::nblocks_of(0xFFFFFFFFull * 64, 4) == 0xFFFFFFFFu && blm::nblocks_of(0xFFFFFFFFull * 64 + 1, 4) == 0 &&
            blm::nblocks_of(1ull << 40, 64) == 0 && blm::nblocks_of(~0ull, 64) == 0,
        "2^32 blocks or more: no filter");
  Entries e;
  std::vector<std::string> ks;
  for (uint32_t n = 0; n <= 24; ++n) {
    std::string k;
    for (uint32_t j = 0; j < n; ++j) k.push_back((char)((7 * n + 3 * j + 1) % 251));
    e.push_back({k, "len-" + std::to_string(n)});
  }
  std::sort(e.begin(), e.end());
  for (auto& kv : e) {
    around(&ks, kv.first);
    if (!kv.first.empty()) {
      std::string x = kv.first;
      x.back() = (char)(x.back() ^ 0x80);
      ks.push_back(x);
    }
  }
  Batch b;
  b.add_table(data_image(e), items_image(items_of(e, 7)));
  b.set_keys(ks);
  check_all(b, "key lengths");
}

static void test_empty() {
  Batch b;
  b.set_keys({"a", ""});
  check_all(b, "no tables");
  Batch c;
  c.add_table("", items_image({}));
  c.set_keys({});
  check_all(c, "no queries");
  Batch d;  // the empty table's filter is one zero block: every pair is dropped
  d.add_table("", items_image({}));
  d.add_table(data_image({{"only", "one"}}), items_image({{"only", 0}}));
  d.set_keys({"", "a", "only", "onlx", "only\0"});
  const Counts k = check(d, "degenerate", 256, 12);
  CHECK(k.tables == 2 && k.keys == 3, "degenerate: an empty table and a table of one record (%llu, %llu)",
        (unsigned long long)k.tables, (unsigned long long)k.keys);
}

int main() {
  static_assert(sizeof(blm::Desc) == 16, "the filter's descriptor");
  test_lengths();
  test_random();
  test_doctored();
  test_interleaved();
  test_empty();
  CHECK(total_bloomed > 1000, "the filters drop pairs (%llu)", (unsigned long long)total_bloomed);
  if (fails) {
    printf("%d failure(s)\n", fails);
    return 1;
  }
  printf("bloom ok\n");
  return 0;
}
