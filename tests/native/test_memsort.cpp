// Host model of the batch memtable build (csrc/lsmck_memsort.h): the whole
// refinement the kernels of lsmck_memtable.hip run -- validate, the rounds of
// chunk_tail / stable sort by (group, chunk, tail) / regroup over the active
// positions, resolve and the mem_bytes shares -- with std::stable_sort in
// place of the device's radix sort, compared with a std::map that replays the
// commands one by one as MemTable::from_log does.  Built with
// -fsanitize=address,undefined: the key arena is an exact-size heap block, 4
// byte aligned and a multiple of 4 long (what a device allocation gives the
// kernel), with keys flush against both ends, so a dword loaded that holds no
// byte of the arena is caught.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "lsmck_memsort.h"

using namespace lsmck;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

struct Built {
  std::vector<uint32_t> src;  // the live entries' commands, in key order
  uint64_t bytes = 0;
  long rounds = 0;
};

// the kernels' steps, slot by slot
static Built build(const uint8_t* keys, const std::vector<lsmck_wal_cmd>& cmds) {
  const uint64_t n = cmds.size();
  Built out;
  if (!n) return out;
  std::vector<uint32_t> perm(n), grp(n, 0), apos(n);
  std::vector<uint8_t> head(n, 1);
  for (uint64_t i = 0; i < n; ++i) perm[i] = apos[i] = (uint32_t)i;
  uint64_t m = n >= 2 ? n : 0;
  for (uint64_t r = 0; m; ++r, ++out.rounds) {
    std::vector<uint64_t> chunk(m);
    std::vector<uint32_t> tail(m), g(m), idx(m), o(m), hd(m), act(m), next;
    for (uint64_t j = 0; j < m; ++j) {  // mem_chunk
      const uint32_t p = apos[j], c = perm[p];
      const mem::ChunkTail ct = mem::chunk_tail(keys, cmds[c].key_off, cmds[c].klen, r);
      chunk[j] = ct.chunk, tail[j] = ct.tail, g[j] = grp[p], idx[j] = c, o[j] = (uint32_t)j;
    }
    // three stable passes, the least significant field first
    std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return tail[a] < tail[b]; });
    std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return chunk[a] < chunk[b]; });
    if (r) std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return g[a] < g[b]; });
    for (uint64_t i = 0; i < m; ++i) {  // mem_bound + the max-scan
      const bool b = i == 0 || !mem::same_run(g[o[i]], chunk[o[i]], tail[o[i]], g[o[i - 1]], chunk[o[i - 1]], tail[o[i - 1]]);
      hd[i] = b ? (uint32_t)i : hd[i - 1];
    }
    std::vector<uint32_t> nperm(m), ngrp(m);
    for (uint64_t i = 0; i < m; ++i) {  // mem_regroup
      const bool first = hd[i] == i, last = i + 1 == m || hd[i + 1] == i + 1;
      nperm[i] = idx[o[i]];
      ngrp[i] = apos[hd[i]];
      head[apos[i]] = first ? 1 : 0;
      act[i] = mem::stays_active(tail[o[i]], !(first && last)) ? 1u : 0u;
    }
    for (uint64_t i = 0; i < m; ++i) {
      perm[apos[i]] = nperm[i], grp[apos[i]] = ngrp[i];
      if (act[i]) next.push_back(apos[i]);  // mem_compact
    }
    if (next.size() > m) abort();
    apos = next;
    m = next.size();
  }
  int64_t bytes = 0;
  for (uint64_t p = 0; p < n; ++p) {  // mem_resolve, mem_emit
    bytes += mem::contribution(cmds.data(), perm.data(), head.data(), p);
    if (mem::live(cmds.data(), perm.data(), head.data(), n, p)) out.src.push_back(perm[p]);
  }
  if (bytes < 0) abort();
  out.bytes = (uint64_t)bytes;
  return out;
}

// MemTable::from_log (memtable.rs:28-47)
static Built replay(const uint8_t* keys, const std::vector<lsmck_wal_cmd>& cmds) {
  std::map<std::string, uint32_t> map;  // key -> the command that wrote it (std::string orders as unsigned bytes)
  int64_t bytes = 0;
  for (uint32_t i = 0; i < cmds.size(); ++i) {
    const lsmck_wal_cmd& c = cmds[i];
    const std::string k((const char*)keys + c.key_off, c.klen);
    if (c.type == 1u) {
      map[k] = i;
      bytes += (int64_t)c.klen + c.vlen;
    } else {
      auto it = map.find(k);
      if (it != map.end()) {
        bytes -= (int64_t)c.klen + cmds[it->second].vlen;
        map.erase(it);
      }
    }
  }
  Built out;
  for (auto& kv : map) out.src.push_back(kv.second);
  out.bytes = (uint64_t)bytes;
  return out;
}

// an exact-size arena, 4-byte aligned and a multiple of 4 long
struct Arena {
  uint8_t* p;
  uint32_t size;
  explicit Arena(uint32_t sz) : size(sz) {
    if (posix_memalign((void**)&p, 4 > sizeof(void*) ? 4 : sizeof(void*), sz ? sz : 4)) abort();
  }
  ~Arena() { free(p); }
};

static int check(const char* what, const uint8_t* keys, uint64_t kb, const std::vector<lsmck_wal_cmd>& cmds,
                 long rounds = -1) {
  for (size_t i = 0; i < cmds.size(); ++i)
    if (!mem::valid(cmds[i], kb, 1u << 20)) return printf("FAIL %s: a valid command was refused (%zu)\n", what, i), 1;
  const Built a = build(keys, cmds), b = replay(keys, cmds);
  if (a.src != b.src || a.bytes != b.bytes)
    return printf("FAIL %s: %zu entries / %llu bytes, expected %zu / %llu\n", what, a.src.size(),
                  (unsigned long long)a.bytes, b.src.size(), (unsigned long long)b.bytes), 1;
  for (size_t j = 1; j < a.src.size(); ++j) {  // the order is sst::key_less's
    const lsmck_wal_cmd &x = cmds[a.src[j - 1]], &y = cmds[a.src[j]];
    if (!sst::key_less(keys + x.key_off, x.klen, keys + y.key_off, y.klen)) return printf("FAIL %s: key_less\n", what), 1;
  }
  if (rounds >= 0 && a.rounds != rounds) return printf("FAIL %s: %ld rounds, expected %ld\n", what, a.rounds, rounds), 1;
  return 0;
}

static lsmck_wal_cmd cmd(uint32_t type, uint64_t ko, uint32_t kl, uint32_t vl = 0) {
  lsmck_wal_cmd c;
  c.key_off = ko, c.val_off = 0, c.klen = kl, c.vlen = vl, c.type = type, c.reserved = 0;
  return c;
}

// two keys of `len` bytes, back to back, filling the arena: equal, or different in the last byte
static int pair(uint32_t len, bool equal, long rounds) {
  Arena A(2 * len);
  for (uint32_t i = 0; i < len; ++i) A.p[i] = A.p[len + i] = (uint8_t)(i * 37u + 1u);
  if (!equal && len) A.p[2 * len - 1] ^= 0x80u;
  char what[64];
  snprintf(what, sizeof what, "pair %u %s", len, equal ? "equal" : "last byte");
  return check(what, A.p, A.size, {cmd(1, 0, len, 3), cmd(1, len, len, 5)}, rounds);
}

int main() {
  int fails = 0;
  // the round counts of the issue's model
  fails += pair(8, true, 1);
  fails += pair(16, true, 2);
  fails += pair(0, true, 1);
  fails += pair(40, true, 5);
  {
    Arena A(44);  // two 9-byte keys equal in 8 bytes | an 8-byte key and its 9-byte extension
    memset(A.p, 7, 44);
    A.p[8] = 1, A.p[17] = 2;
    fails += check("nine/nine", A.p, 44, {cmd(1, 0, 9), cmd(1, 9, 9)}, 2);
    fails += check("eight/nine", A.p, 44, {cmd(1, 20, 9), cmd(1, 20, 8)}, 1);
    fails += check("one", A.p, 44, {cmd(2, 0, 9)}, 0);
    fails += check("none", A.p, 44, {}, 0);
  }
  {
    Arena A(84);  // two 41-byte keys that differ in the last byte, flush against both ends (1 + 41 + 41 + 1)
    for (uint32_t i = 0; i < 84; ++i) A.p[i] = (uint8_t)(i % 41u);
    memmove(A.p + 43, A.p + 2, 41);
    memmove(A.p, A.p + 2, 41);
    A.p[83] ^= 1u;
    fails += check("forty-one", A.p, 84, {cmd(1, 0, 41), cmd(1, 43, 41)}, 6);
  }
  // the contract's corners
  {
    lsmck_wal_cmd c = cmd(1, 0, 4, 4);
    fails += !mem::valid(c, 4, 4);
    c.key_off = 1, fails += mem::valid(c, 4, 4);
    c.key_off = 0, c.val_off = 1, fails += mem::valid(c, 4, 4);
    c.type = 2, fails += !mem::valid(c, 4, 4);  // a Remove's value range is not looked at
    c.type = 0, fails += mem::valid(c, 4, 4);
    c.type = 3, fails += mem::valid(c, 4, 4);
    c = cmd(1, ~0ull, 0, 0), c.val_off = ~0ull, fails += !mem::valid(c, 0, 0);  // empty ranges lie anywhere
    c = cmd(1, ~0ull, 1, 0), fails += mem::valid(c, 16, 0);
    if (fails) printf("FAIL: valid()\n");
  }
  // keys of every length 0..26 at every start residue, at the arena's first and last byte
  for (uint32_t len = 0; len <= 26; ++len)
    for (uint32_t res = 0; res < 8; ++res) {
      const uint32_t size = (res + 2 * len + 3u) & ~3u;
      Arena A(size);
      for (uint32_t i = 0; i < size; ++i) A.p[i] = (uint8_t)(rnd() >> 7 | 1u);
      if (len) memcpy(A.p + size - len, A.p + res, len);  // the last key equals the first ...
      std::vector<lsmck_wal_cmd> c = {cmd(1, res, len, 1), cmd(1, size - len, len, 2)};
      fails += check("flush equal", A.p, size, c, (long)(len / 8 + (len % 8 || !len ? 1 : 0)));
      if (len) {
        A.p[size - 1] ^= 0xFFu;  // ... but for its last byte
        fails += check("flush last byte", A.p, size, c, (long)((len - 1) / 8 + 1));
      }
    }
  // random logs over a small alphabet: prefixes and near-prefixes of one another, overwrites and removes
  const uint8_t alpha[5] = {0, 1, 0x7F, 0x80, 0xFF};
  for (int it = 0; it < 3000; ++it) {
    const uint32_t size = 4u * (1u + below(12)), n = below(it % 10 ? 40 : 400);
    Arena A(size);
    const uint32_t kinds = 1u + below(5);
    for (uint32_t i = 0; i < size; ++i) A.p[i] = alpha[below(kinds)];
    std::vector<lsmck_wal_cmd> c;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t kl = below(it % 3 ? std::min(12u, size + 1u) : size + 1u), ko = below(size - kl + 1u);
      c.push_back(cmd(below(4) ? 1u : 2u, ko, kl, below(9)));
    }
    if (check("random", A.p, size, c)) {
      ++fails;
      break;
    }
  }
  // the adapter (rec_to_cmd)
  {
    lsmck_wal_rec16 r = {100, 4, 10};
    lsmck_wal_cmd c = mem::rec_to_cmd(r, 200);
    fails += !(c.key_off == 100 && c.val_off == 104 && c.klen == 4 && c.vlen == 10 && c.type == 1 && c.reserved == 0);
    c = mem::rec_to_cmd(r, 110);  // cut inside the value
    fails += !(c.klen == 4 && c.vlen == 6 && mem::valid(c, 110, 110));
    c = mem::rec_to_cmd(r, 104);  // the value gone
    fails += !(c.klen == 4 && c.vlen == 0 && mem::valid(c, 104, 104));
    c = mem::rec_to_cmd(r, 103);  // cut inside the key
    fails += mem::valid(c, 103, 103);
    r = {100, 0xFFFFFFF0u, 0x20u};  // klen + vlen wraps to 16
    c = mem::rec_to_cmd(r, 200);
    fails += mem::valid(c, 200, 200);
    r = {100 | LSMCK_WAL_REC16_REMOVE, 8, 0};
    c = mem::rec_to_cmd(r, 200);
    fails += !(c.type == 2 && c.klen == 8 && c.key_off == 100 && mem::valid(c, 200, 200));
    c = mem::rec_to_cmd(r, 105);  // a Remove's key is all the payload read
    fails += !(c.type == 2 && c.klen == 5 && mem::valid(c, 105, 105));
    if (fails) printf("FAIL: rec_to_cmd or before\n");
  }
  if (fails) return printf("memsort FAILED (%d)\n", fails), 1;
  printf("memsort ok\n");
  return 0;
}
