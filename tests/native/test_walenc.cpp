// Host model of the batch WAL encode's gather (csrc/lsmck_walenc.h): the code
// the kernel wal_encode_gather runs per tile and per chunk -- the 64-probe
// search of the tile's first record, the slice of record offsets, the chunk's
// fast and bytewise paths -- run here lane by lane over random batches, at
// several image alignments, and compared with a plain encoder.  Built with
// -fsanitize=address,undefined: arenas and image are exact-size heap blocks,
// so a load outside a source's dwords or a store outside the image is caught.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "lsmck_walenc.h"

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

// one batch: maxlen bounds key and value lengths; returns the failures found
static int run(size_t n, uint32_t maxk, uint32_t maxv, uint32_t shift, bool shared) {
  const size_t kb = 4 * ((maxk + 4099) / 4), vb = shared ? kb : 4 * ((maxv + 4099) / 4);
  uint8_t* keys = (uint8_t*)malloc(kb);  // (sizes are multiples of 4: a source's last dword ends inside)
  uint8_t* vals = shared ? keys : (uint8_t*)malloc(vb);
  for (size_t i = 0; i < kb; ++i) keys[i] = (uint8_t)rnd();
  if (!shared)
    for (size_t i = 0; i < vb; ++i) vals[i] = (uint8_t)rnd();
  std::vector<lsmck_wal_cmd> cmds(n);
  std::vector<uint64_t> off(n + 1);
  std::vector<uint8_t> want;
  uint64_t run_off = 0;
  for (size_t i = 0; i < n; ++i) {
    lsmck_wal_cmd& c = cmds[i];
    c.type = below(4) == 0 ? 2u : 1u;
    c.klen = below(8) == 0 ? 0u : below(maxk + 1);
    c.vlen = below(8) == 0 ? 0u : below(std::min<uint32_t>(maxv, (uint32_t)vb) + 1);
    c.key_off = below((uint32_t)(kb - c.klen + 1));
    c.val_off = below((uint32_t)(vb - c.vlen + 1));
    c.reserved = 0;
    if (c.type == 2 && below(2)) c.val_off = ~0ull, c.vlen = 0xFFFFFFFFu;  // a Remove's value fields are not looked at
    const uint64_t sz = enc::rec_size(c, kb, vb);
    if (!sz) return printf("FAIL: a valid command was refused (i=%zu)\n", i), 1;
    off[i] = run_off;
    run_off += sz;
    want.push_back((uint8_t)c.type);
    put32(want, 0);  // the CRC field: the stamp's
    put32(want, c.klen);
    if (c.type == 1) put32(want, c.vlen);
    want.insert(want.end(), keys + c.key_off, keys + c.key_off + c.klen);
    if (c.type == 1) want.insert(want.end(), vals + c.val_off, vals + c.val_off + c.vlen);
  }
  off[n] = run_off;
  const int64_t total = (int64_t)run_off;
  if ((size_t)total != want.size()) return printf("FAIL: sizes\n"), 1;
  // the image: exact end (the sanitizer's), `shift` guard bytes in front (checked)
  uint8_t* buf = (uint8_t*)malloc((size_t)total + shift);
  memset(buf, 0xAA, (size_t)total + shift);
  uint8_t* img = buf + shift;
  std::vector<uint8_t> written((size_t)total, 0);
  const uint64_t base = (uintptr_t)img & (enc::kTile - 1u);
  const uint64_t tiles = (base + (uint64_t)total + enc::kTile - 1u) / enc::kTile;
  std::vector<enc::slice_t> srel(enc::kSlice + 1u);
  std::vector<lsmck_wal_cmd> cache(enc::kCache);
  int fails = 0;
  for (uint64_t k = 0; k < tiles; ++k) {
    enc::Tile t;
    t.keys = keys, t.vals = vals, t.cmds = cmds.data(), t.total = total;
    t.ts = (int64_t)(k * enc::kTile) - (int64_t)base;
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
    const uint64_t r0 = (uint64_t)(std::upper_bound(off.begin(), off.begin() + n, (uint64_t)t0) - off.begin()) - 1;
    if (lo != r0) return printf("FAIL: first record %llu, want %llu\n", (unsigned long long)lo, (unsigned long long)r0), 1;
    t.r0 = lo;
    t.off0 = (int64_t)off[lo];
    srel[0] = 0;
    t.N = 1;
    for (uint32_t b = 0; b < enc::kSlice; b += enc::kBlock) {
      uint32_t last = 0;
      for (uint32_t tid = 0; tid < enc::kBlock; ++tid) {
        last = enc::slice_entry(off.data(), n, t.r0, 1u + b + tid, t.ts);
        srel[1u + b + tid] = (enc::slice_t)last;
      }
      t.N += enc::kBlock;
      if (!(last < enc::kTile)) break;
    }
    // every record that starts inside the tile is in the slice
    for (uint64_t r = r0 + 1; r < n && (int64_t)off[r] < t.ts + (int64_t)enc::kTile; ++r)
      if (r - r0 >= t.N || srel[r - r0] != (enc::slice_t)((int64_t)off[r] - t.ts)) return printf("FAIL: slice misses record %llu\n", (unsigned long long)r), 1;
    for (uint32_t tid = 0; tid < enc::kCache; ++tid) {
      memset(&cache[tid], 0xEE, sizeof cache[tid]);  // (the kernel leaves these unwritten; they are never read)
      if (t.r0 + tid < n) cache[tid] = cmds[t.r0 + tid];
    }
    for (uint32_t tid = 0; tid < enc::kBlock; ++tid)  // the kernel's loop, lane by lane
      for (uint32_t p = tid * 16u; p < enc::kTile; p += enc::kGroup * enc::kBlock * 16u)
        enc::chunks(t, (const enc::slice_t*)srel.data(), (const lsmck_wal_cmd*)cache.data(), p, enc::kBlock * 16u, img);
    for (uint32_t p = 0; p < enc::kTile; p += 16u) {  // which image bytes a chunk owns
      const enc::Span sp = enc::span_of(t, p);
      for (uint32_t b = sp.b0; b < sp.b1; ++b) written[(size_t)(sp.pos + b)]++;
    }
  }
  for (int64_t q = 0; q < total; ++q) {
    if (written[(size_t)q] != 1 && fails++ < 5) printf("FAIL: byte %lld owned by %u chunks\n", (long long)q, written[(size_t)q]);
    if (img[q] != want[(size_t)q] && fails++ < 5) printf("FAIL: byte %lld is %02x, want %02x (n=%zu shift=%u)\n", (long long)q, img[q], want[(size_t)q], n, shift);
  }
  for (uint32_t g = 0; g < shift; ++g)
    if (buf[g] != 0xAA && fails++ < 5) printf("FAIL: guard byte %u written\n", g);
  // payload descriptors: lengths, places, and the empty payloads' rule
  uint64_t prev_o = 0;
  uint32_t prev_l = 0;
  for (size_t i = 0; i < n; ++i) {
    uint32_t len;
    const uint64_t o = enc::payload_desc(cmds.data(), off.data(), i, &len);
    const uint32_t wl = cmds[i].klen + (cmds[i].type == 1 ? cmds[i].vlen : 0);
    if (len != wl || (len && o != off[i] + enc::hdr(cmds[i].type))) fails++;
    if (!len && i > 0 && prev_l && o != prev_o + prev_l && fails++ < 5) printf("FAIL: empty payload %zu not at its predecessor's end\n", i);
    if (!len && i > 0 && !prev_l && o != prev_o) {  // a run: the same place, for the first 8 of it
      size_t k = i;
      while (k > 0 && cmds[k - 1].klen + (cmds[k - 1].type == 1 ? cmds[k - 1].vlen : 0) == 0) --k;
      if (i - k < 8 && fails++ < 5) printf("FAIL: empty payload %zu of a run moved\n", i);
    }
    prev_o = o, prev_l = len;
  }
  free(buf);
  if (!shared) free(vals);
  free(keys);
  return fails;
}

int main() {
  int fails = 0;
  // invalid commands
  lsmck_wal_cmd c = {0, 0, 4, 4, 1, 0};
  fails += enc::rec_size(c, 4, 4) != 21;
  c.type = 0, fails += enc::rec_size(c, 4, 4) != 0;
  c.type = 3, fails += enc::rec_size(c, 4, 4) != 0;
  c.type = 1, c.klen = 0xFFFFFFFFu, c.vlen = 1, fails += enc::rec_size(c, ~0ull, ~0ull) != 0;
  c.klen = 4, c.vlen = 4, c.key_off = 1, fails += enc::rec_size(c, 4, 4) != 0;
  c.key_off = 0, c.val_off = 1, fails += enc::rec_size(c, 4, 4) != 0;
  c.type = 2, fails += enc::rec_size(c, 4, 4) != 13;  // a Remove's value is not looked at
  c.key_off = ~0ull, fails += enc::rec_size(c, 4, 4) != 0;
  c.klen = 0, fails += enc::rec_size(c, 4, 4) != 9;  // an empty key reaches nothing
  // sizes past 2^32: the header is added in 64 bits
  c = {0, 0, 0xFFFFFFFFu, 0, 1, 0};
  fails += enc::rec_size(c, ~0ull, ~0ull) != 13ull + 0xFFFFFFFFull;
  c = {0, 0, 0xFFFFFFF7u, 0, 2, 0};
  fails += enc::rec_size(c, ~0ull, ~0ull) != 9ull + 0xFFFFFFF7ull;
  c = {0, 0, 0xFFFFFFFFu, 0, 2, 0};
  fails += enc::rec_size(c, ~0ull, ~0ull) != 9ull + 0xFFFFFFFFull;
  c = {0, 0, 1, 0xFFFFFFFEu, 1, 0};
  fails += enc::rec_size(c, ~0ull, ~0ull) != 13ull + 0xFFFFFFFFull;
  if (fails) printf("FAIL: rec_size\n");
  const uint32_t shifts[] = {0, 1, 3, 15, 16, 17, 4097};
  for (uint32_t s : shifts) {
    fails += run(1, 0, 0, s, false);
    fails += run(2, 1, 1, s, false);
    fails += run(20000, 3, 2, s, false);     // records of 9..18 bytes: three to a chunk
    fails += run(20000, 48, 48, s, true);    // short keys and values at every alignment, one arena
    fails += run(3000, 70, 900, s, false);   // chunks inside values
    fails += run(40, 4000, 70000, s, false); // values longer than a tile
  }
  if (fails) return printf("walenc: %d failures\n", fails), 1;
  printf("walenc ok\n");
  return 0;
}
