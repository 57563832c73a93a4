// Host model of the batch Db::get (csrc/lsmck_dbget.h, with csrc/lsmck_sstget.h
// for the tables): the steps the kernels of lsmck_dbget.hip run, in their
// order -- the run pass, the index pass and the queries' check, every (query,
// run) pair and then every (query, table) pair with the winner's minimum (the
// pairs in both orders), resolve and the lengths' scan, and the gather's tile
// loop lane by lane (the wave's 64-probe search, the slice, every lane's
// chunks; the slice form and the form that searches off[] itself) -- compared
// with a std::map per source and a loop over bytes.  Built with
// -fsanitize=address,undefined: every arena is an exact-size heap block whose
// start is 4-byte aligned and whose length is a multiple of 4 (what a device
// allocation gives the aligned-dword loads), with keys and values flush
// against both ends, and `out` ends flush with its block, so a byte read or
// written outside is caught.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "lsmck_dbget.h"

using namespace lsmck;
typedef std::vector<std::pair<std::string, std::string>> Entries;

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

struct Heap {  // an exact-size block
  uint8_t* p;
  size_t n;
  explicit Heap(const std::string& s) : n(s.size()) {
    p = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(p, s.data(), n);
  }
  Heap(const Heap&) = delete;
  ~Heap() { free(p); }
};
// filler in front so that the payload starts near residue `res` and the block is whole dwords
static std::string front_for(size_t res, size_t payload, char fill) {
  return std::string(res + (4 - (res + payload) % 4) % 4, fill);
}
static void put(std::string& s, uint64_t x, int bytes) {
  for (int b = 0; b < bytes; ++b) s.push_back((char)(x >> (8 * b)));
}

// ---- a run: two arenas (or one) and its entries ----------------------------------
struct RunSpec {
  Entries e;
  size_t kres = 0, vres = 0;
  bool one = false;
};
struct RunMem {
  Heap *keys, *vals;
  std::vector<lsmck_wal_cmd>* ents;  // (a heap block of exactly nent entries)
  lsmck_get_run d;
  explicit RunMem(const RunSpec& s) {
    std::string k, v;
    ents = new std::vector<lsmck_wal_cmd>();
    size_t kb = 0, vb = 0;
    for (auto& x : s.e) kb += x.first.size(), vb += x.second.size();
    if (s.one) {
      k = front_for(s.kres, kb + vb, (char)0xCC);
      for (auto& x : s.e) {
        ents->push_back({k.size(), k.size() + x.first.size(), (uint32_t)x.first.size(), (uint32_t)x.second.size(), 1u, 0u});
        k += x.first + x.second;
      }
    } else {
      k = front_for(s.kres, kb, (char)0xCC), v = front_for(s.vres, vb, (char)0xBB);
      for (auto& x : s.e) {
        ents->push_back({k.size(), v.size(), (uint32_t)x.first.size(), (uint32_t)x.second.size(), 1u, 0u});
        k += x.first, v += x.second;
      }
    }
    ents->shrink_to_fit();
    keys = new Heap(k);
    vals = s.one ? keys : new Heap(v);
    d.keys = keys->p, d.keys_bytes = keys->n, d.vals = vals->p, d.vals_bytes = vals->n;
    d.ents = ents->data(), d.nent = ents->size();
  }
  RunMem(const RunMem&) = delete;
  ~RunMem() {
    if (vals != keys) delete vals;
    delete keys;
    delete ents;
  }
};

// ---- tables: written as the reference writes them (index of every step-th key) ----
struct Tables {
  std::string data, index;
  std::vector<lsmck_sstable_span> spans;
  std::vector<std::map<std::string, std::string>> ref;
  void front(size_t n) { data.assign(n, (char)0xEE); }
  void add(const Entries& t, uint32_t step) {
    std::string d, x;
    std::vector<std::pair<std::string, uint64_t>> items;
    for (size_t i = 0; i < t.size(); ++i) {
      if (i % step == 0) items.push_back({t[i].first, d.size()});
      put(d, t[i].first.size(), 4), put(d, t[i].second.size(), 4);
      d += t[i].first + t[i].second;
    }
    put(x, items.size(), 8);
    for (auto& it : items) put(x, it.first.size(), 8), x += it.first, put(x, it.second, 8);
    spans.push_back({data.size(), d.size(), index.size(), x.size()});
    data += d, index += x;
    ref.push_back(std::map<std::string, std::string>(t.begin(), t.end()));
  }
};

// ---- the gather, lane by lane ------------------------------------------------------
struct GatherStats {
  uint64_t tiles = 0, slice_tiles = 0, global_tiles = 0;
};
static void gather(const uint64_t* off, const uint64_t* src, uint64_t n, uint8_t* out, bool force_global,
                   GatherStats* S) {
  const uint64_t total = off[n];
  if (!n || !total) return;
  const uint64_t tiles = (((uintptr_t)out & (dbg::kTile - 1u)) + total + dbg::kTile - 1u) / dbg::kTile;
  for (uint64_t blk = 0; blk < tiles; ++blk) {
    std::vector<dbg::slice_t> srel(dbg::kSlice + 1u, 0);
    std::vector<uint64_t> cache(dbg::kCache, 0);
    dbg::Tile t;
    t.off = off, t.src = src, t.n = n;
    t.total = (int64_t)total;
    t.ts = (int64_t)blk * dbg::kTile - (int64_t)((uintptr_t)out & (dbg::kTile - 1u));
    const int64_t t0 = t.ts > 0 ? t.ts : 0;
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
      uint32_t c = 0;
      bool prev = true;
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint64_t idx = enc::probe(lo, hi, lane);
        const bool le = idx < hi && (int64_t)off[idx] <= t0;
        CHECK(prev || !le, "the probes that hold are the first lanes");
        prev = le, c += le;
      }
      enc::narrow(lo, hi, c);
    }
    CHECK((int64_t)off[lo] <= t0 && t0 < (int64_t)off[lo + 1], "the tile's first value owns its first byte");
    t.r0 = lo, t.off0 = (int64_t)off[lo];
    for (uint32_t tid = 0; tid < dbg::kBlock; ++tid)
      if (t.r0 + tid < n) cache[tid] = src[t.r0 + tid];
    t.N = 1;
    bool whole = false;
    for (uint32_t base = 0; base < dbg::kSlice; base += dbg::kBlock) {
      uint32_t v = 0;
      for (uint32_t tid = 0; tid < dbg::kBlock; ++tid) {
        v = dbg::slice_entry(off, n, t.r0, 1u + base + tid, t.ts);
        srel[1u + base + tid] = (dbg::slice_t)v;
      }
      t.N += dbg::kBlock;
      if (!(v < dbg::kTile)) {
        whole = true;
        break;
      }
    }
    ++S->tiles;
    if (whole && !force_global) {
      ++S->slice_tiles;
      dbg::Slice rel;
      rel.s = srel.data();
      for (uint32_t tid = 0; tid < dbg::kBlock; ++tid)
        for (uint32_t p = tid * 16u; p < dbg::kTile; p += dbg::kGroup * dbg::kBlock * 16u)
          dbg::chunks(t, rel, (const uint64_t*)cache.data(), p, dbg::kBlock * 16u, out);
    } else {
      ++S->global_tiles;
      t.N = n - t.r0 + 1u;
      for (uint32_t tid = 0; tid < dbg::kBlock; ++tid)
        for (uint32_t p = tid * 16u; p < dbg::kTile; p += dbg::kGroup * dbg::kBlock * 16u)
          dbg::chunks(t, dbg::Global(), (const uint64_t*)cache.data(), p, dbg::kBlock * 16u, out);
    }
  }
}

// `out` at residue `res` of a tile-aligned address, ending flush with its block; the bytes in front are a guard
struct OutBlock {
  uint8_t *base, *out;
  size_t res, total;
  OutBlock(size_t res_, size_t total_) : res(res_), total(total_) {
    void* q = nullptr;
    if (posix_memalign(&q, dbg::kTile, res + total ? res + total : 1)) exit(2);
    base = (uint8_t*)q, out = base + res;
    memset(base, 0xAA, res + total);
  }
  OutBlock(const OutBlock&) = delete;
  ~OutBlock() { free(base); }
  bool guard() const {
    for (size_t i = 0; i < res; ++i)
      if (base[i] != 0xAA) return false;
    return true;
  }
};

// values (src, len) -> out, against a loop over bytes; both forms of the slice
static GatherStats check_gather(const std::vector<std::pair<const uint8_t*, uint64_t>>& vals, size_t res, const char* what) {
  const uint64_t n = vals.size();
  GatherStats S;
  std::vector<uint64_t>* off = new std::vector<uint64_t>(n + 1, 0);
  std::vector<uint64_t>* src = new std::vector<uint64_t>(n, 0);
  for (uint64_t i = 0; i < n; ++i) {
    (*off)[i + 1] = (*off)[i] + vals[i].second;
    (*src)[i] = vals[i].second ? (uint64_t)(uintptr_t)vals[i].first : 0xDEAD0000DEAD0000ull;  // (a zero-length value's is not read)
  }
  const uint64_t total = (*off)[n];
  for (int form = 0; form < 2; ++form) {
    OutBlock O(res, (size_t)total);
    gather(off->data(), src->data(), n, O.out, form == 1, &S);
    CHECK(O.guard(), "%s: no byte in front of out is written", what);
    uint64_t at = 0, bad = 0;
    for (uint64_t i = 0; i < n && !bad; ++i)
      for (uint64_t b = 0; b < vals[i].second; ++b, ++at)
        if (O.out[at] != vals[i].first[b]) {
          bad = 1;
          CHECK(false, "%s (form %d, residue %zu): value %llu byte %llu", what, form, res, (unsigned long long)i,
                (unsigned long long)b);
          break;
        }
  }
  delete off;
  delete src;
  return S;
}

static std::string bytes_of(size_t n, uint32_t tag) {
  std::string s(n, 0);
  for (size_t j = 0; j < n; ++j) s[j] = (char)((tag * 37u + j * 7u + j / 251u) % 253u + 1u);
  return s;
}

static void gather_tests() {
  const size_t lens[] = {0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 32767, 32768, 32769, 65537};
  // every length alone and among neighbours, the source at every residue 0..15, out at every residue
  for (size_t res = 0; res < 16; ++res) {
    std::string arena(res, (char)0x11);  // (the block is 16-byte aligned: the first value lies at residue res)
    std::vector<std::pair<size_t, size_t>> at;
    uint32_t tag = (uint32_t)res;
    for (size_t L : lens) {
      at.push_back({arena.size(), L});
      arena += bytes_of(L, tag++);
      arena += std::string((res * 5 + L) % 7, (char)0x22);  // (the next one at another residue)
    }
    // ... and one value flush with the arena's end, the block whole dwords
    const size_t last = 40 + (4 - (arena.size() + 40) % 4) % 4;
    at.push_back({arena.size(), last});
    arena += bytes_of(last, 99);
    Heap A(arena);
    std::vector<std::pair<const uint8_t*, uint64_t>> vals;
    for (auto& x : at) vals.push_back({A.p + x.first, x.second});
    check_gather(vals, res, "every length");
    check_gather(vals, dbg::kTile - 16 + res, "every length, out near a tile's end");
    for (auto& v : vals) check_gather({v}, (res * 3 + 1) % 16, "one value");
    std::reverse(vals.begin(), vals.end());
    check_gather(vals, 15 - res, "every length, reversed");
  }
  // runs of zero-length answers at the start, in the middle and at the end; totals under 16 and of 0
  {
    const std::string v = bytes_of(100, 7);
    Heap A(v);
    typedef std::vector<std::pair<const uint8_t*, uint64_t>> V;
    const std::pair<const uint8_t*, uint64_t> z{nullptr, 0}, a{A.p, 5}, b{A.p + 5, 20}, c{A.p + 25, 75};
    check_gather(V{z, z, z, a, z, z, b, z, c, z, z, z}, 3, "zero-length runs");
    check_gather(V{z, a, z}, 9, "a total under 16");
    check_gather(V{a, {A.p + 5, 3}, {A.p + 8, 7}}, 15, "a total of 15 across a chunk");
    check_gather(V{z, z, z}, 0, "a total of 0");
    check_gather(V{}, 0, "no value");
    // more zero-length values inside one tile than the slice holds: off[] itself is searched
    V many;
    many.push_back(b);
    for (int i = 0; i < 5000; ++i) many.push_back(z);
    many.push_back(c);
    for (int i = 0; i < 300; ++i) many.push_back(i % 3 ? z : a);
    const GatherStats S = check_gather(many, 5, "5000 zero-length values in a tile");
    CHECK(S.global_tiles >= 2 && S.slice_tiles == 0, "that tile does not fit the slice (%llu, %llu)",
          (unsigned long long)S.global_tiles, (unsigned long long)S.slice_tiles);
  }
  // random values, many small ones (several to a chunk) and a few long
  for (int round = 0; round < 12; ++round) {
    const std::string v = bytes_of(70000 + below(999) * 4, 1000 + round);
    Heap A(v);
    std::vector<std::pair<const uint8_t*, uint64_t>> vals;
    const uint32_t nv = 1 + below(400);
    for (uint32_t i = 0; i < nv; ++i) {
      const uint32_t kind = below(10);
      const uint64_t L = kind < 2 ? 0 : kind < 7 ? below(9) : kind < 9 ? below(300) : below(70000);
      const uint64_t o = below((uint32_t)(A.n - L + 1));
      vals.push_back({A.p + (i == 0 ? A.n - L : i == 1 ? 0 : o), L});
    }
    const GatherStats S = check_gather(vals, below(dbg::kTile), "random values");
    CHECK(S.tiles == S.slice_tiles + S.global_tiles, "every tile takes one form");
  }
}

// ---- the whole call ------------------------------------------------------------------
struct Out {
  std::vector<lsmck_get_result> res;
  std::vector<uint64_t> off;
  std::string out;
  uint64_t bad_run_entry = ~0ull, bad_table = ~0ull, bad_query = ~0ull;
  uint64_t run_skipped = 0, tab_skipped = 0;
};

static Out run_call(const std::vector<lsmck_get_run>& runs, const uint8_t* data, uint64_t db, const uint8_t* index,
                    uint64_t ib, const std::vector<lsmck_sstable_span>& spans, const uint8_t* qkeys, uint64_t qb,
                    const std::vector<lsmck_get_query>& q, bool reversed, size_t out_res) {
  const uint64_t nrun = runs.size(), ntab = spans.size(), n = q.size();
  Out O;
  // 1. dbg_run_pass
  std::vector<uint64_t> rf(nrun + 1, 0);
  for (uint64_t r = 0; r < nrun; ++r) rf[r + 1] = rf[r] + runs[r].nent;
  std::vector<mrg::OKey> rok(rf[nrun] + 1);
  for (uint64_t x = 0; x < rf[nrun]; ++x) {
    const uint64_t e = reversed ? rf[nrun] - 1 - x : x;
    if (!dbg::run_pass(runs.data(), rf.data(), nrun, e, rok.data())) O.bad_run_entry = std::min(O.bad_run_entry, e);
  }
  // 2. the index pass (the serial parse; the parallel one: tests/native/test_sstget.cpp) and the queries
  std::vector<uint64_t> first(ntab + 1, 0);
  for (uint64_t t = 0; t < ntab; ++t) {
    const lsmck_sstable_span s = spans[t];
    uint64_t c = get::kNo;
    if (mrg::span_ok(s.data_off, s.data_len, db) && s.data_len <= mrg::kMaxTable && mrg::span_ok(s.index_off, s.index_len, ib))
      c = get::index_parse(index + s.index_off, s.index_len, nullptr, 0);
    if (c == get::kNo) O.bad_table = std::min<uint64_t>(O.bad_table, t), c = 0;
    first[t + 1] = first[t] + c;
  }
  std::vector<uint64_t> ioff(first[ntab] + 1), ipos(first[ntab] + 1);
  std::vector<mrg::OKey> iok(first[ntab] + 1), qok(n);
  std::vector<uint32_t> win(n);
  if (O.bad_table == ~0ull)
    for (uint64_t t = 0; t < ntab; ++t) {
      const uint8_t* idx = index + spans[t].index_off;
      const uint64_t k = first[t + 1] - first[t];
      CHECK(get::index_parse(idx, spans[t].index_len, ioff.data() + first[t], k) == k, "the parse fills the offsets");
      for (uint64_t sl = first[t]; sl < first[t + 1]; ++sl) {
        iok[sl] = get::item_okey(idx, ioff[sl]), ipos[sl] = get::item_pos(idx, ioff[sl]);
        if (sl > first[t] && !get::item_less(idx, ioff[sl - 1], ioff[sl])) O.bad_table = std::min<uint64_t>(O.bad_table, t);
      }
    }
  for (uint64_t i = 0; i < n; ++i) {
    mrg::OKey k{0, 0, 0};
    if (get::query_ok(q[i], qb)) k = get::key_of(qkeys, q[i].key_off, q[i].klen).ok;
    else O.bad_query = std::min<uint64_t>(O.bad_query, i);
    qok[i] = k, win[i] = get::kNoTable;
  }
  if (O.bad_run_entry != ~0ull || O.bad_table != ~0ull || O.bad_query != ~0ull) return O;  // (dbg_failed)
  auto run = [&](uint64_t r) { return dbg::run_of(runs[r], rok.data() + rf[r]); };
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
  // 3. dbg_probe, then 4. get_probe with base = nrun: the pairs in one order or the other
  for (uint64_t x = 0; x < n * nrun; ++x) {
    const uint64_t w = reversed ? n * nrun - 1 - x : x, r = w / n, i = w - r * n;
    if (r > win[i]) {
      ++O.run_skipped;
      continue;
    }
    uint64_t at;
    if (dbg::run_get(run(r), key(i), &at)) win[i] = std::min<uint32_t>(win[i], (uint32_t)r);
  }
  for (uint64_t x = 0; x < n * ntab; ++x) {
    const uint64_t w = reversed ? n * ntab - 1 - x : x, t = w / n, i = w - t * n;
    if (nrun + t > win[i]) {
      ++O.tab_skipped;
      continue;
    }
    uint64_t vpos;
    uint32_t vlen;
    bool walked;
    if (get::table_get(table(t), key(i), &vpos, &vlen, &walked)) win[i] = std::min<uint32_t>(win[i], (uint32_t)(nrun + t));
  }
  // 5. dbg_resolve and the scan
  O.res.resize(n);
  std::vector<uint64_t>* len = new std::vector<uint64_t>(n + 1, 0);
  std::vector<uint64_t>* src = new std::vector<uint64_t>(n, 0);
  for (uint64_t i = 0; i < n; ++i) {
    lsmck_get_result x = get::result_none();
    const uint32_t s = win[i];
    if (s < nrun) {
      const dbg::Run R = run(s);
      uint64_t at;
      const bool some = dbg::run_get(R, key(i), &at);
      CHECK(some, "resolve finds what the run probe found (query %llu)", (unsigned long long)i);
      if (some) x = dbg::run_result(R, R.ents[at], s), (*src)[i] = (uint64_t)(uintptr_t)(R.vals + R.ents[at].val_off);
    } else if (s != get::kNoTable) {
      const get::Table T = table(s - nrun);
      uint64_t vpos;
      uint32_t vlen;
      const bool some = get::table_get(T, key(i), &vpos, &vlen, nullptr);
      CHECK(some, "resolve finds what the table probe found (query %llu)", (unsigned long long)i);
      if (some) x = get::result_of(T.img, spans[s - nrun].data_off, vpos, vlen, s), (*src)[i] = (uint64_t)(uintptr_t)(T.img + vpos);
    }
    O.res[i] = x;
    (*len)[i] = dbg::answered_len(x);
  }
  uint64_t acc = 0;
  for (uint64_t i = 0; i <= n; ++i) {
    const uint64_t l = i < n ? (*len)[i] : 0;
    (*len)[i] = acc, acc += l;
  }
  // 6. dbg_gather
  OutBlock B(out_res, (size_t)(*len)[n]);
  GatherStats S;
  gather(len->data(), src->data(), n, B.out, false, &S);
  CHECK(B.guard(), "no byte in front of out is written");
  O.off = *len;
  O.out.assign((const char*)B.out, (size_t)(*len)[n]);
  delete len;
  delete src;
  return O;
}

struct Case {
  std::vector<RunSpec> runs;
  Tables tabs;
  std::vector<std::string> keys;
  size_t qres = 0;
};

static Out check(const Case& c, const char* what, uint64_t want_run = ~0ull, uint64_t want_tab = ~0ull,
                 uint64_t want_query = ~0ull, const std::vector<lsmck_get_query>* q_override = nullptr,
                 std::vector<std::vector<lsmck_wal_cmd>>* ents_override = nullptr) {
  std::vector<RunMem*> mem;
  std::vector<lsmck_get_run> runs;
  std::vector<std::vector<lsmck_wal_cmd>*> keep;
  for (size_t r = 0; r < c.runs.size(); ++r) {
    mem.push_back(new RunMem(c.runs[r]));
    lsmck_get_run d = mem.back()->d;
    if (ents_override) {
      keep.push_back(new std::vector<lsmck_wal_cmd>((*ents_override)[r]));
      keep.back()->shrink_to_fit();
      d.ents = keep.back()->data(), d.nent = keep.back()->size();
    }
    runs.push_back(d);
  }
  // the data arena in whole dwords, its last table flush with the end
  std::string data = c.tabs.data;
  std::vector<lsmck_sstable_span> spans = c.tabs.spans;
  const size_t lead = (4 - data.size() % 4) % 4;
  data = std::string(lead, (char)0xEE) + data;
  for (auto& s : spans) s.data_off += lead;
  size_t kb = 0;
  for (auto& k : c.keys) kb += k.size();
  std::string qkeys = front_for(c.qres, kb, (char)0xDD);
  std::vector<lsmck_get_query> q;
  for (auto& k : c.keys) q.push_back({qkeys.size(), (uint32_t)k.size(), 0u}), qkeys += k;
  if (q_override) q = *q_override;
  Heap D(data), X(c.tabs.index), K(qkeys);
  Out O = run_call(runs, D.p, D.n, X.p, X.n, spans, K.p, K.n, q, false, c.qres % 16);
  CHECK(O.bad_run_entry == want_run, "%s: bad_run_entry %llu, want %llu", what, (unsigned long long)O.bad_run_entry,
        (unsigned long long)want_run);
  if (want_run == ~0ull) CHECK(O.bad_table == want_tab, "%s: bad_table %llu", what, (unsigned long long)O.bad_table);
  if (want_run == ~0ull && want_tab == ~0ull)
    CHECK(O.bad_query == want_query, "%s: bad_query %llu", what, (unsigned long long)O.bad_query);
  if (want_run == ~0ull && want_tab == ~0ull && want_query == ~0ull) {
    const Out R = run_call(runs, D.p, D.n, X.p, X.n, spans, K.p, K.n, q, true, 16 - c.qres % 16);
    CHECK(R.res.size() == O.res.size() && (O.res.empty() || !memcmp(R.res.data(), O.res.data(), 16 * O.res.size())),
          "%s: the pairs' order changes nothing", what);
    CHECK(R.out == O.out && R.off == O.off, "%s: nor does it change the gather", what);
    // the model: a std::map per source, a loop over bytes
    std::string want_out;
    for (size_t i = 0; i < c.keys.size(); ++i) {
      const std::string* v = nullptr;
      uint32_t source = get::kNoTable;
      for (size_t r = 0; r < c.runs.size() && !v; ++r) {
        for (auto& e : c.runs[r].e)
          if (e.first == c.keys[i]) v = &e.second, source = (uint32_t)r;
      }
      for (size_t t = 0; t < c.tabs.ref.size() && !v; ++t) {
        auto hit = c.tabs.ref[t].find(c.keys[i]);
        if (hit != c.tabs.ref[t].end()) v = &hit->second, source = (uint32_t)(c.runs.size() + t);
      }
      const lsmck_get_result g = O.res[i];
      CHECK(g.table == source, "%s: query %zu source %u, want %u", what, i, g.table, source);
      if (!v) {
        CHECK(g.val_off == 0 && g.vlen == 0, "%s: query %zu: a miss is all zero", what, i);
        continue;
      }
      const bool tomb = *v == std::string(1, '\0');
      CHECK(g.vlen == v->size() && (g.val_off >> 63) == (tomb ? 1u : 0u), "%s: query %zu length / tombstone", what, i);
      const uint8_t* arena = source < c.runs.size() ? runs[source].vals : D.p;
      const uint64_t o = g.val_off & ~LSMCK_GET_TOMBSTONE;
      CHECK(v->empty() || !memcmp(arena + o, v->data(), v->size()), "%s: query %zu: val_off names the value", what, i);
      if (source < c.runs.size() && v->empty()) CHECK(o == 0, "%s: an empty run value's offset is 0", what);
      if (!tomb) want_out += *v;
      CHECK(O.off[i + 1] - O.off[i] == (tomb ? 0 : v->size()), "%s: query %zu answered length", what, i);
    }
    CHECK(O.out == want_out, "%s: the gathered values", what);
  } else {
    CHECK(O.res.empty() && O.out.empty(), "%s: no result on an error", what);
  }
  for (auto m : mem) delete m;
  for (auto k : keep) delete k;
  return O;
}

static const char* B24 = "ABCDEFGHIJKLMNOPQRSTUVWX";
static Entries run_entries(uint32_t m, uint32_t seed) {
  std::map<std::string, std::string> e;
  std::vector<std::string> special;
  for (uint32_t n = 0; n < 18; ++n) special.push_back(std::string(B24, n));
  special.push_back(std::string(B24, 24)), special.push_back(std::string(B24, 24) + "!");
  for (const char* t : {"tie-a", "tie-b", "tie-a!", "\x80", "\xff\xff"}) special.push_back(std::string(B24, 8) + t);
  special.push_back(std::string(B24, 8) + std::string(1, '\0'));
  special.push_back(std::string("\0", 1)), special.push_back(std::string("\0\1", 2)), special.push_back("\1");
  for (uint32_t i = 0; e.size() < m; ++i) {
    std::string k = i < special.size() ? special[(i + seed) % special.size()] : "r" + std::to_string(1000 + i * 7 + seed) + std::string(i % 19, 'y');
    const uint32_t kind = (uint32_t)e.size() % 5;
    e[k] = kind == 0 ? std::string(1, '\0') : kind == 1 ? "" : bytes_of(1 + (i * 13 + seed) % 40, i + seed);
  }
  return Entries(e.begin(), e.end());
}
static std::vector<std::string> queries_for(const Entries& e) {
  std::vector<std::string> q;
  for (auto& x : e) {
    q.push_back(x.first);
    q.push_back(x.first + std::string(1, '\0'));  // a key plus one byte
    if (!x.first.empty()) {
      q.push_back(x.first.substr(0, x.first.size() - 1));  // a prefix
      std::string b = x.first;
      b.back() = (char)((uint8_t)b.back() - 1), b += "\xff\xff";
      if ((uint8_t)x.first.back() != 0) q.push_back(b);  // just below
    }
  }
  q.push_back(""), q.push_back(std::string(19, '\xff'));
  return q;
}

static void call_tests() {
  // run sizes 0, 1, 2, 63, 64, 65 at every residue of both arenas, alone and in front of a table
  const uint32_t sizes[] = {0, 1, 2, 63, 64, 65};
  for (uint32_t res = 0; res < 16; ++res)
    for (uint32_t m : sizes) {
      Case c;
      RunSpec r;
      r.e = run_entries(m, res), r.kres = res, r.vres = (res * 7 + 3) % 16, r.one = res % 4 == 3;
      c.runs.push_back(r);
      c.keys = queries_for(r.e);
      c.qres = res;
      check(c, "one run");
      if (res % 4 == 1) {
        Entries t = run_entries(40, res + 5);
        for (auto& x : t) x.second = "T" + x.second;
        c.tabs.front(res);
        c.tabs.add(t, 1 + res % 7);
        for (auto& k : queries_for(t)) c.keys.push_back(k);
        check(c, "a run in front of a table");
      }
    }
  // precedence: the same key in run 0, run 1 and table 0; tombstones on either side; an empty value; a duplicate
  {
    Case c;
    const std::string tomb(1, '\0');
    RunSpec r0, r1;
    r0.e = {{"all", "from-run0"}, {"dead", tomb}, {"empty", ""}, {"live", "again"}};
    r1.e = {{"all", "from-run1"}, {"live", tomb}, {"old", "run1-only"}, {"olddead", tomb}};
    r0.kres = 3, r0.vres = 5, r1.kres = 1, r1.one = true;
    c.runs = {r0, r1};
    c.tabs.front(3);
    c.tabs.add({{"all", "from-table0"}, {"dead", "alive-in-table"}, {"tab", "table-only"}, {"tabdead", tomb}}, 100);
    c.tabs.add({{"old", "shadowed"}, {"tab", "older"}, {"tabdead", "older-live"}}, 2);
    c.keys = {"all", "dead", "live", "empty", "miss", "all", "old", "olddead", "tab", "tabdead", "", "miss"};
    const Out O = check(c, "precedence");
    CHECK(O.out == "from-run0againfrom-run0run1-onlytable-only", "precedence: the gathered arena");
    CHECK(O.res[1].table == 0 && O.res[9].table == 2 && O.res[6].table == 1, "precedence: the sources");
    // no runs; no tables; nothing at all; no queries
    Case t = c;
    t.runs.clear();
    check(t, "no runs");
    Case r = c;
    r.tabs = Tables();
    check(r, "no tables");
    r.runs.clear();
    check(r, "no sources");
    c.keys.clear();
    check(c, "no queries");
  }
  // refusals: equal neighbours, a decreasing pair, a range outside its run's arena, a type 2; the first one counts,
  // across the runs; run before table before query
  {
    Case c;
    RunSpec r0, r1;
    r0.e = run_entries(10, 0), r1.e = run_entries(12, 2), r1.one = true;
    c.runs = {r0, r1};
    c.tabs.add(run_entries(5, 3), 2);
    c.keys = queries_for(r0.e);
    auto ents = [&](void) {
      std::vector<std::vector<lsmck_wal_cmd>> v;
      for (auto& r : c.runs) {
        RunMem m(r);
        v.push_back(*m.ents);
      }
      return v;
    };
    std::vector<std::vector<lsmck_wal_cmd>> e = ents();
    e[1][4] = e[1][3];
    check(c, "equal neighbours", 10 + 4, ~0ull, ~0ull, nullptr, &e);
    e = ents();
    std::swap(e[0][6], e[0][7]);
    check(c, "a decreasing pair", 7, ~0ull, ~0ull, nullptr, &e);
    e = ents();
    e[1][11].vlen += 1;  // (the last value of the shared arena: one byte past it)
    check(c, "a value past its arena", 10 + 11, ~0ull, ~0ull, nullptr, &e);
    e = ents();
    e[0][2].key_off = ~0ull - 1;
    check(c, "a key offset past its arena", 2, ~0ull, ~0ull, nullptr, &e);
    e = ents();
    e[1][0].type = 2u;
    e[1][5].klen = 0xFFFFFFFFu;
    check(c, "type 2 before a length", 10, ~0ull, ~0ull, nullptr, &e);
    e = ents();
    CHECK(e[0][0].klen == 0, "run 0 starts with the empty key");
    e[0][0].key_off = ~0ull;  // (an empty key's offset is not looked at)
    check(c, "an empty key's offset", ~0ull, ~0ull, ~0ull, nullptr, &e);
    // all three at once
    Case b = c;
    b.tabs.index[0] ^= 1;  // (the count is off by one: the parse fails)
    std::vector<lsmck_get_query> q;
    size_t at = 0, kb = 0;
    for (auto& k : c.keys) kb += k.size();
    at = front_for(0, kb, 0).size();
    for (auto& k : c.keys) q.push_back({at, (uint32_t)k.size(), 0u}), at += k.size();
    q[3].reserved = 1;
    e = ents();
    e[1][2].type = 0;
    check(b, "run, table and query", 12, ~0ull, ~0ull, &q, &e);
    check(b, "table and query", ~0ull, 0, ~0ull, &q, nullptr);
    check(c, "query", ~0ull, ~0ull, 3, &q, nullptr);
  }
  // seeded: two runs and several tables over one key range
  for (int round = 0; round < 6; ++round) {
    Case c;
    auto draw = [&](uint32_t m, const char* tag) {
      std::map<std::string, std::string> e;
      while (e.size() < m) {
        const uint32_t x = below(700);
        const uint32_t kind = below(8);
        e["key" + std::to_string(100000 + x) + std::string(x % 5, 's')] =
            kind == 0 ? std::string(1, '\0') : kind == 1 ? "" : tag + bytes_of(below(kind == 2 ? 5000 : 60), x);
      }
      return Entries(e.begin(), e.end());
    };
    RunSpec r0, r1;
    r0.e = draw(100 + below(50), "a"), r1.e = draw(150, "b");
    r0.kres = below(16), r0.vres = below(16), r1.kres = below(16), r1.one = round % 2 == 0;
    c.runs = {r0, r1};
    c.tabs.front(below(16));
    for (int t = 0; t < 4; ++t) c.tabs.add(draw(60 + below(80), "t"), 1 + below(12));
    for (int i = 0; i < 700; ++i) {
      const uint32_t x = below(760);
      c.keys.push_back("key" + std::to_string(100000 + x) + std::string((x + (i % 9 == 0)) % 5, 's'));
    }
    c.qres = below(16);
    const Out O = check(c, "seeded");
    CHECK(O.tab_skipped > 0 && O.run_skipped > 0, "a source behind a winner is skipped");
  }
}

int main() {
  gather_tests();
  call_tests();
  if (fails) {
    printf("dbget: %d failures\n", fails);
    return 1;
  }
  printf("dbget ok\n");
  return 0;
}
