// Host model of the batch SSTable encode's data gather (csrc/lsmck_sstenc.h):
// the code the kernel sst_gather runs per tile and per chunk -- the 64-probe
// search of the tile's first record, the slice of record offsets, the chunk's
// fast and bytewise paths -- run here lane by lane, at several image
// alignments, and compared byte for byte with a plain serial writer; and the
// record arithmetic and the key order.  Built with
// -fsanitize=address,undefined, once with the kernel's tile and once with
// -DLSMCK_SST_TILE=256u: arenas and image are exact-size heap blocks, so a
// load outside a source's dwords or a store outside the image is caught.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "lsmck_sstenc.h"

using namespace lsmck;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

static void put32(std::vector<uint8_t>& v, uint32_t x) {
  for (int b = 0; b < 4; ++b) v.push_back((uint8_t)(x >> (8 * b)));
}

// Encode the entries with the tile logic at an image base `shift` bytes past
// a block's start (`lead` more bytes of the block lie before the image and
// are guard bytes, as are `trail` behind it) and compare.
static int encode(const std::vector<lsmck_wal_cmd>& cmds, const uint8_t* keys, uint64_t kb, const uint8_t* vals,
                  uint64_t vb, uint32_t shift) {
  const size_t n = cmds.size();
  std::vector<uint64_t> off(n + 1);
  std::vector<uint8_t> want;
  uint64_t run_off = 0;
  for (size_t i = 0; i < n; ++i) {
    const lsmck_wal_cmd& c = cmds[i];
    const uint64_t sz = sst::rec_size(c, kb, vb);
    if (!sz) return printf("FAIL: a valid entry was refused (i=%zu)\n", i), 1;
    off[i] = run_off;
    run_off += sz;
    put32(want, c.klen);  // the plain serial writer (datafile.rs:27-35)
    put32(want, c.vlen);
    want.insert(want.end(), keys + c.key_off, keys + c.key_off + c.klen);
    want.insert(want.end(), vals + c.val_off, vals + c.val_off + c.vlen);
  }
  off[n] = run_off;
  const int64_t total = (int64_t)run_off;
  if ((size_t)total != want.size()) return printf("FAIL: sizes\n"), 1;
  if (total == 0) return 0;  // (no tile: the launcher returns before the kernel)
  // the image: exact end (the sanitizer's), `shift` guard bytes in front (checked)
  // (the block starts on a tile: the image's base is exactly `shift` past one)
  void* blk = nullptr;
  if (posix_memalign(&blk, sst::kTile, (size_t)total + shift)) return printf("FAIL: posix_memalign\n"), 1;
  uint8_t* buf = (uint8_t*)blk;
  memset(buf, 0xAA, (size_t)total + shift);
  uint8_t* img = buf + shift;
  std::vector<uint8_t> written((size_t)total, 0);
  const uint64_t base = (uintptr_t)img & (sst::kTile - 1u);
  const uint64_t tiles = (base + (uint64_t)total + sst::kTile - 1u) / sst::kTile;
  std::vector<sst::slice_t> srel(sst::kSlice + 1u);
  std::vector<lsmck_wal_cmd> cache(sst::kCache);
  int fails = 0;
  for (uint64_t k = 0; k < tiles; ++k) {
    sst::Tile t;
    t.keys = keys, t.vals = vals, t.cmds = cmds.data(), t.total = total;
    t.ts = (int64_t)(k * sst::kTile) - (int64_t)base;
    const int64_t t0 = t.ts > 0 ? t.ts : 0;
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
      uint32_t c = 0;
      bool prefix = true;
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint64_t idx = enc::probe(lo, hi, lane);
        const bool le = idx < hi && (int64_t)off[idx] <= t0;
        if (le && !prefix) return printf("FAIL: probes not monotone\n"), 1;
        prefix = prefix && le;
        c += le;
      }
      const uint64_t span = hi - lo;
      enc::narrow(lo, hi, c);
      if (hi - lo >= span) return printf("FAIL: search does not narrow\n"), 1;
    }
    // the kernel's r0: some record with off[r0] <= t0 < off[hi]; with records
    // of 8 bytes and more, offsets are distinct, so it is the last such one
    const uint64_t r0 = (uint64_t)(std::upper_bound(off.begin(), off.begin() + n, (uint64_t)t0) - off.begin()) - 1;
    if (lo != r0) return printf("FAIL: first record %llu, want %llu\n", (unsigned long long)lo, (unsigned long long)r0), 1;
    t.r0 = lo;
    t.off0 = (int64_t)off[lo];
    srel[0] = 0;
    t.N = 1;
    for (uint32_t b = 0; b < sst::kSlice; b += sst::kBlock) {
      uint32_t last = 0;
      for (uint32_t tid = 0; tid < sst::kBlock; ++tid) {
        last = sst::slice_entry(off.data(), n, t.r0, 1u + b + tid, t.ts);
        srel[1u + b + tid] = (sst::slice_t)last;
      }
      t.N += sst::kBlock;
      if (!(last < sst::kTile)) break;
    }
    // every record that starts inside the tile is in the slice
    for (uint64_t r = r0 + 1; r < n && (int64_t)off[r] < t.ts + (int64_t)sst::kTile; ++r)
      if (r - r0 >= t.N || srel[r - r0] != (sst::slice_t)((int64_t)off[r] - t.ts))
        return printf("FAIL: slice misses record %llu\n", (unsigned long long)r), 1;
    for (uint32_t tid = 0; tid < sst::kCache; ++tid) {
      memset(&cache[tid], 0xEE, sizeof cache[tid]);  // (the kernel leaves these unwritten; they are never read)
      if (t.r0 + tid < n) cache[tid] = cmds[t.r0 + tid];
    }
    for (uint32_t tid = 0; tid < sst::kBlock; ++tid)  // the kernel's loop, lane by lane
      for (uint32_t p = tid * 16u; p < sst::kTile; p += sst::kGroup * sst::kBlock * 16u)
        sst::chunks(t, (const sst::slice_t*)srel.data(), (const lsmck_wal_cmd*)cache.data(), p, sst::kBlock * 16u, img);
    for (uint32_t p = 0; p < sst::kTile; p += 16u) {  // which image bytes a chunk owns
      const enc::Span sp = sst::span_of(t, p);
      for (uint32_t b = sp.b0; b < sp.b1; ++b) written[(size_t)(sp.pos + b)]++;
    }
  }
  for (int64_t q = 0; q < total; ++q) {
    if (written[(size_t)q] != 1 && fails++ < 5) printf("FAIL: byte %lld owned by %u chunks\n", (long long)q, written[(size_t)q]);
    if (img[q] != want[(size_t)q] && fails++ < 5)
      printf("FAIL: byte %lld is %02x, want %02x (n=%zu shift=%u)\n", (long long)q, img[q], want[(size_t)q], n, shift);
  }
  for (uint32_t g = 0; g < shift; ++g)
    if (buf[g] != 0xAA && fails++ < 5) printf("FAIL: guard byte %u written\n", g);
  free(buf);
  return fails;
}

// random entries: maxk / maxv bound key and value lengths
static int run(size_t n, uint32_t maxk, uint32_t maxv, uint32_t shift, bool shared) {
  const size_t kb = 4 * ((maxk + 4099) / 4), vb = shared ? kb : 4 * ((maxv + 4099) / 4);
  uint8_t* keys = (uint8_t*)malloc(kb);  // (sizes are multiples of 4: a source's last dword ends inside)
  uint8_t* vals = shared ? keys : (uint8_t*)malloc(vb);
  for (size_t i = 0; i < kb; ++i) keys[i] = (uint8_t)rnd();
  if (!shared)
    for (size_t i = 0; i < vb; ++i) vals[i] = (uint8_t)rnd();
  std::vector<lsmck_wal_cmd> cmds(n);
  for (size_t i = 0; i < n; ++i) {
    lsmck_wal_cmd& c = cmds[i];
    c.type = 1;
    c.klen = below(8) == 0 ? 0u : below(maxk + 1);
    c.vlen = below(8) == 0 ? 0u : below(std::min<uint32_t>(maxv, (uint32_t)vb) + 1);
    c.key_off = below((uint32_t)(kb - c.klen + 1));
    c.val_off = below((uint32_t)(vb - c.vlen + 1));
    c.reserved = 0;
  }
  const int fails = encode(cmds, keys, kb, vals, vb, shift);
  if (!shared) free(vals);
  free(keys);
  return fails;
}

// every key and value length 0..48 at every source residue mod 16, each
// source in a 64-byte slot of its own
static int sweep(uint32_t shift) {
  const size_t n = 2 * 49 * 16, kb = n * 64;
  uint8_t* keys = (uint8_t*)malloc(kb);
  uint8_t* vals = (uint8_t*)malloc(kb);
  for (size_t i = 0; i < kb; ++i) keys[i] = (uint8_t)rnd(), vals[i] = (uint8_t)rnd();
  std::vector<lsmck_wal_cmd> cmds(n);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t len = (uint32_t)(i % 784) / 16u, res = (uint32_t)i % 16u;
    lsmck_wal_cmd& c = cmds[i];
    c.type = 1, c.reserved = 0;
    c.klen = i < 784 ? len : below(49);
    c.vlen = i < 784 ? below(49) : len;
    c.key_off = i * 64 + (i < 784 ? res : below(16));
    c.val_off = i * 64 + (i < 784 ? below(16) : res);
  }
  const int fails = encode(cmds, keys, kb, vals, kb, shift);
  free(vals);
  free(keys);
  return fails;
}

static int smallest(uint32_t shift) {
  uint8_t* keys = (uint8_t*)malloc(4);
  uint8_t* vals = (uint8_t*)malloc(4);
  memcpy(keys, "kKkK", 4), memcpy(vals, "vVvV", 4);
  int fails = 0;
  const uint32_t kv[4][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}};
  for (auto& s : kv) {
    std::vector<lsmck_wal_cmd> one = {{0, 0, s[0], s[1], 1, 0}};
    fails += encode(one, keys, 4, vals, 4, shift);
  }
  std::vector<lsmck_wal_cmd> two = {{0, 0, 0, 0, 1, 0}, {0, 0, 0, 0, 1, 0}};  // two 8-byte records: one chunk
  fails += encode(two, keys, 4, vals, 4, shift);
  std::vector<lsmck_wal_cmd> none;
  fails += encode(none, keys, 4, vals, 4, shift);
  free(vals);
  free(keys);
  return fails;
}

static bool less(const char* a, const char* b) {
  return sst::key_less((const uint8_t*)a, (uint32_t)strlen(a), (const uint8_t*)b, (uint32_t)strlen(b));
}

int main() {
  int fails = 0;
  // invalid entries
  lsmck_wal_cmd c = {0, 0, 4, 4, 1, 0};
  fails += sst::rec_size(c, 4, 4) != 16;
  c.type = 0, fails += sst::rec_size(c, 4, 4) != 0;
  c.type = 2, fails += sst::rec_size(c, 4, 4) != 0;
  c.type = 1, c.key_off = 1, fails += sst::rec_size(c, 4, 4) != 0;
  c.key_off = 0, c.val_off = 1, fails += sst::rec_size(c, 4, 4) != 0;
  c.val_off = ~0ull, fails += sst::rec_size(c, 4, 4) != 0;
  c.vlen = 0, fails += sst::rec_size(c, 4, 4) != 12;  // an empty value reaches nothing
  c.key_off = ~0ull, c.klen = 0, fails += sst::rec_size(c, 4, 4) != 8;
  // the size limit: 8 + klen + vlen <= 2^32-1
  c = {0, 0, 0xFFFFFFF7u, 0, 1, 0};
  fails += sst::rec_size(c, ~0ull, ~0ull) != 0xFFFFFFFFull;
  c = {0, 0, 0xFFFFFFF8u, 0, 1, 0};
  fails += sst::rec_size(c, ~0ull, ~0ull) != 0;
  c = {0, 0, 0xFFFFFFF0u, 8, 1, 0};
  fails += sst::rec_size(c, ~0ull, ~0ull) != 0;
  c = {0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 1, 0};
  fails += sst::rec_size(c, ~0ull, ~0ull) != 0;
  if (fails) printf("FAIL: rec_size\n");
  // key order: bytewise, a proper prefix first, bytes above 0x7f last; the
  // dword path (aligned keys of 4 bytes and more) and the byte path agree
  alignas(4) static const char k[][12] = {"", "a", "ab", "abcd", "abcdabcd", "abcdabce", "abce", "abd", "b", "\xff\x01\x02\x03", "\xff\xff\xff\xff\x01"};
  const int nk = (int)(sizeof k / sizeof k[0]);
  for (int i = 0; i < nk; ++i)
    for (int j = 0; j < nk; ++j) {
      if (less(k[i], k[j]) != (i < j) && fails++ < 5) printf("FAIL: key_less(%d, %d)\n", i, j);
      char u[2][16];  // the same keys one byte off alignment
      strcpy(u[0] + 1, k[i]), strcpy(u[1] + 1, k[j]);
      if (less(u[0] + 1, u[1] + 1) != (i < j) && fails++ < 5) printf("FAIL: key_less unaligned (%d, %d)\n", i, j);
    }
  fails += sst::index_count(0) != 0 || sst::index_count(1) != 1 || sst::index_count(100) != 1 ||
           sst::index_count(101) != 2 || sst::index_count(201) != 3;
  // image bases 0, 1, 3 and 15 past a tile, and more
  const uint32_t shifts[] = {0, 1, 3, 15, 16, 17, 4097};
  for (uint32_t s : shifts) {
    fails += smallest(s);
    fails += sweep(s);
    fails += run(2, 1, 1, s, false);
    fails += run(20000, 3, 2, s, false);     // records of 8..13 bytes: up to three to a chunk
    fails += run(20000, 48, 48, s, true);    // short keys and values at every alignment, one arena
    fails += run(3000, 70, 900, s, false);   // chunks inside values
    fails += run(40, 4000, 70000, s, false); // values longer than a tile
  }
  if (fails) return printf("sstenc: %d failures\n", fails), 1;
  printf("sstenc ok (tile %u)\n", sst::kTile);
  return 0;
}
