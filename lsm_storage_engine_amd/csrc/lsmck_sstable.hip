// lsmck_sstable.hip -- batch SSTable encode on the GPU (gfx950):
// lsmck_sstable_encode_batch, the write-side counterpart of
// lsmck_checksums_verify_many.  The batch form of SsTable::from_memtable's
// file writes (src/tokio/sstable.rs:84-129; datafile.rs:27-35,
// sstable_index.rs:42-46): entries (key and value ranges in two arenas), cut
// into tables by table_first, become the tables' data files, back to back in
// one arena, and their bincode index files, back to back in another.
//   1. sst_size + the u64 scan: every entry's record size (8 + klen + vlen)
//      and validity -> off[0..n]; the scan's three passes are sst_scan_a, the
//      WAL file's wal_seg_scan_b, sst_scan_c (any u64 array, in place);
//   2. sst_first + sst_order: byte flags of the tables' first entries, then a
//      thread per other entry compares its key with its predecessor's;
//   3. sst_index_size + the same scan: the index items' places; sst_spans:
//      every table's span in both arenas, the digests' descriptors, the first
//      table too long to hash;
//      -- the totals and the two error words are read back here, once --
//   4. sst_gather: the data arena, output-centric (lsmck_sstenc.h);
//   5. sst_index_write: a thread per index item (about 1 % of the entries);
//   6. the digests: the batch SHA-256 dispatcher over each arena, a
//      descriptor per table (lsmck_api.cpp).
// The record arithmetic, the key order and the gather's tile logic:
// lsmck_sstenc.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsmck.h"
#include "lsmck_device.h"
#include "lsmck_sstenc.h"

namespace lsmck {

#define SST_SCAN_ITEMS 4u
#define SST_SCAN_BLOCK 1024u

__device__ __forceinline__ uint64_t sst_wave_incl_scan(uint64_t x, uint32_t lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = __shfl_up(x, d, 64);
    if (lane >= (uint32_t)d) x += o;
  }
  return x;
}

// 1. off[i] = entry i's record size (0: invalid); info[0] = the first invalid entry
__global__ __launch_bounds__(256) void sst_size(const lsmck_wal_cmd* __restrict__ ents, uint64_t n, uint64_t kb,
                                                 uint64_t vb, uint64_t* __restrict__ off,
                                                 unsigned long long* __restrict__ info) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t sz = sst::rec_size(ents[i], kb, vb);
  off[i] = sz;
  if (!sz) atomicMin(info, (unsigned long long)i);
}

// exclusive scan of v[0..n) in place, v[n] = the total (also to *total)
__global__ __launch_bounds__(SST_SCAN_BLOCK) void sst_scan_a(const uint64_t* __restrict__ v, uint64_t n,
                                                              uint64_t* __restrict__ bsum) {
  __shared__ uint64_t s[SST_SCAN_BLOCK / 64];
  const uint64_t i0 = ((uint64_t)blockIdx.x * SST_SCAN_BLOCK + threadIdx.x) * SST_SCAN_ITEMS;
  uint64_t x = 0;
  for (uint32_t j = 0; j < SST_SCAN_ITEMS; ++j)
    if (i0 + j < n) x += v[i0 + j];
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  if ((threadIdx.x & 63u) == 0) s[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
    for (uint32_t k = 0; k < SST_SCAN_BLOCK / 64; ++k) t += s[k];
    bsum[blockIdx.x] = t;
  }
}
__global__ __launch_bounds__(SST_SCAN_BLOCK) void sst_scan_c(uint64_t* __restrict__ v, uint64_t n,
                                                              const uint64_t* __restrict__ bsum,
                                                              unsigned long long* __restrict__ total) {
  __shared__ uint64_t s[SST_SCAN_BLOCK / 64];
  const uint64_t i0 = ((uint64_t)blockIdx.x * SST_SCAN_BLOCK + threadIdx.x) * SST_SCAN_ITEMS;
  uint64_t w[SST_SCAN_ITEMS], x = 0;
  for (uint32_t j = 0; j < SST_SCAN_ITEMS; ++j) {
    w[j] = i0 + j < n ? v[i0 + j] : 0ull;
    x += w[j];
  }
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t inc = sst_wave_incl_scan(x, lane);
  if (lane == 63u) s[threadIdx.x >> 6] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t acc = 0;
    for (uint32_t k = 0; k < SST_SCAN_BLOCK / 64; ++k) {
      const uint64_t t = s[k];
      s[k] = acc;
      acc += t;
    }
  }
  __syncthreads();
  uint64_t run = bsum[blockIdx.x] + s[threadIdx.x >> 6] + inc - x;
  for (uint32_t j = 0; j < SST_SCAN_ITEMS; ++j)
    if (i0 + j <= n) {  // (v[n]: the total)
      v[i0 + j] = run;
      if (i0 + j == n) *total = run;
      run += w[j];
    }
}

// 2. first[i] = 1 for every table's first entry (an empty table names its
// successor's first entry again: the same byte, the same value)
__global__ __launch_bounds__(256) void sst_first(const uint64_t* __restrict__ tf, uint64_t ntab, uint64_t n,
                                                  uint8_t* __restrict__ first) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntab) return;
  const uint64_t i = tf[t];
  if (i < n) first[i] = 1;
}
// a thread per entry that is not its table's first: its key against its
// predecessor's (sst::key_less).  An entry that sst_size refused, or whose
// predecessor it did, is skipped: its sources may lie anywhere, and the
// refused entry is reported already.
__global__ __launch_bounds__(256) void sst_order(const lsmck_wal_cmd* __restrict__ ents, uint64_t n,
                                                  const uint8_t* __restrict__ keys, uint64_t kb, uint64_t vb,
                                                  const uint8_t* __restrict__ first,
                                                  unsigned long long* __restrict__ info) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + 1u;
  if (i >= n || first[i]) return;
  const lsmck_wal_cmd a = ents[i - 1], b = ents[i];
  if (!sst::rec_size(a, kb, vb) || !sst::rec_size(b, kb, vb)) return;
  if (!sst::key_less(keys + a.key_off, a.klen, keys + b.key_off, b.klen)) atomicMin(info, (unsigned long long)i);
}

// 3. the index items: item k is table item_tab[k]'s count (item_ent[k] = ~0)
// or its entry item_ent[k]
__global__ __launch_bounds__(256) void sst_index_size(const uint32_t* __restrict__ item_ent, uint64_t nitems,
                                                       const lsmck_wal_cmd* __restrict__ ents,
                                                       uint64_t* __restrict__ ioff) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nitems) return;
  const uint32_t e = item_ent[k];
  ioff[k] = e == 0xFFFFFFFFu ? 8ull : 16ull + ents[e].klen;
}
// every table's spans, the digests' descriptors, and the first table whose
// image is too long for a descriptor (info[2]; hash bit 0: data, bit 1: index)
__global__ __launch_bounds__(256) void sst_spans(const uint64_t* __restrict__ tf, const uint64_t* __restrict__ ibase,
                                                  uint64_t ntab, const uint64_t* __restrict__ off,
                                                  const uint64_t* __restrict__ ioff,
                                                  lsmck_sstable_span* __restrict__ spans, uint64_t* __restrict__ doff,
                                                  uint32_t* __restrict__ dlen, uint64_t* __restrict__ xoff,
                                                  uint32_t* __restrict__ xlen, unsigned hash,
                                                  unsigned long long* __restrict__ info) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntab) return;
  lsmck_sstable_span s;
  s.data_off = off[tf[t]];
  s.data_len = off[tf[t + 1]] - s.data_off;
  s.index_off = ioff[ibase[t]];
  s.index_len = ioff[ibase[t + 1]] - s.index_off;
  spans[t] = s;
  doff[t] = s.data_off, dlen[t] = (uint32_t)s.data_len;
  xoff[t] = s.index_off, xlen[t] = (uint32_t)s.index_len;
  if (((hash & 1u) && s.data_len > 0xFFFFFFFFull) || ((hash & 2u) && s.index_len > 0xFFFFFFFFull))
    atomicMin(info + 2, (unsigned long long)t);
}

// 4. The gather (lsmck_sstenc.h): a workgroup per tile of the data arena, 256
// consecutive chunks per pass of the block -- wal_encode_gather's shape: the
// tile's first record from the 64-probe search of off[] by every wave for
// itself, the offsets of the records that start inside the tile in LDS
// relative to the tile (u16), a block's load at a time until one ends past
// the tile, the commands of the tile's first 256 records beside them.
__global__ __launch_bounds__(sst::kBlock) void sst_gather(const uint8_t* __restrict__ keys,
                                                           const uint8_t* __restrict__ vals,
                                                           const lsmck_wal_cmd* __restrict__ ents, uint64_t n,
                                                           const uint64_t* __restrict__ off,
                                                           uint8_t* __restrict__ img) {
  __shared__ sst::slice_t srel[sst::kSlice + 1u];
  __shared__ lsmck_wal_cmd cache[sst::kCache];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  sst::Tile t;
  t.keys = keys;
  t.vals = vals;
  t.cmds = ents;
  t.total = (int64_t)off[n];
  // (the first tile starts at or before the image: ts <= 0)
  t.ts = (int64_t)blockIdx.x * sst::kTile - (int64_t)((uintptr_t)img & (sst::kTile - 1u));
  const int64_t t0 = t.ts > 0 ? t.ts : 0;
  uint64_t lo = 0, hi = n;  // off[0] = 0 <= t0 < total = off[n]
  while (hi - lo > 1) {     // (wave-uniform)
    const uint64_t idx = enc::probe(lo, hi, lane);
    const bool le = idx < hi && (int64_t)off[idx] <= t0;
    enc::narrow(lo, hi, (uint32_t)__popcll(__ballot(le)));
  }
  t.r0 = lo;
  t.off0 = (int64_t)off[lo];
  if (tid == 0) srel[0] = 0;
  if (t.r0 + tid < n) cache[tid] = ents[t.r0 + tid];
  t.N = 1;
  for (uint32_t base = 0; base < sst::kSlice; base += sst::kBlock) {
    const uint32_t v = sst::slice_entry(off, n, t.r0, 1u + base + tid, t.ts);
    srel[1u + base + tid] = (sst::slice_t)v;
    t.N += sst::kBlock;
    if (!__syncthreads_or(tid == sst::kBlock - 1u && v < sst::kTile)) break;  // (the load's last entry is past the tile)
  }
  for (uint32_t p = tid * 16u; p < sst::kTile; p += sst::kGroup * sst::kBlock * 16u)
    sst::chunks(t, (const sst::slice_t*)srel, (const lsmck_wal_cmd*)cache, p, sst::kBlock * 16u, img);
}

// 5. a thread per index item: the table's count, or klen, the key and the
// record's position in its own table's data file (byte stores: items start
// at any offset)
__device__ __forceinline__ void sst_put64(uint8_t* p, uint64_t x) {
  for (int b = 0; b < 8; ++b) p[b] = (uint8_t)(x >> (8 * b));
}
__global__ __launch_bounds__(256) void sst_index_write(const uint32_t* __restrict__ item_tab,
                                                        const uint32_t* __restrict__ item_ent, uint64_t nitems,
                                                        const uint64_t* __restrict__ tf,
                                                        const lsmck_wal_cmd* __restrict__ ents,
                                                        const uint8_t* __restrict__ keys,
                                                        const uint64_t* __restrict__ off,
                                                        const uint64_t* __restrict__ ioff,
                                                        uint8_t* __restrict__ index) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nitems) return;
  const uint32_t e = item_ent[k], t = item_tab[k];
  uint8_t* p = index + ioff[k];
  if (e == 0xFFFFFFFFu) {
    sst_put64(p, sst::index_count(tf[t + 1] - tf[t]));
    return;
  }
  const lsmck_wal_cmd c = ents[e];
  sst_put64(p, c.klen);
  const uint8_t* src = keys + c.key_off;
  for (uint32_t b = 0; b < c.klen; ++b) p[8u + b] = src[b];
  sst_put64(p + 8u + c.klen, off[e] - off[tf[t]]);
}

}  // namespace lsmck

using namespace lsmck;

static int sst_launch_err() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
static unsigned sst_grid(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

extern "C" uint32_t lsmk_sst_tile(void) { return sst::kTile; }
extern "C" uint64_t lsmk_sst_scan_blocks(uint64_t n) {
  return (n + 1 + SST_SCAN_BLOCK * SST_SCAN_ITEMS - 1) / (SST_SCAN_BLOCK * SST_SCAN_ITEMS);
}
// exclusive scan of v[0..n) in place, v[n] and *total = the sum (bsum: lsmk_sst_scan_blocks(n) entries)
static int sst_scan(uint64_t* v, uint64_t n, uint64_t* bsum, unsigned long long* total, hipStream_t st) {
  const uint32_t nb = (uint32_t)lsmk_sst_scan_blocks(n);
  hipLaunchKernelGGL(sst_scan_a, dim3(nb), dim3(SST_SCAN_BLOCK), 0, st, (const uint64_t*)v, n, bsum);
  int rc = lsmk_scan_u64_blocks(bsum, nb, st);
  if (rc) return rc;
  hipLaunchKernelGGL(sst_scan_c, dim3(nb), dim3(SST_SCAN_BLOCK), 0, st, v, n, (const uint64_t*)bsum, total);
  return sst_launch_err();
}
extern "C" int lsmk_sst_scan(uint64_t* v, uint64_t n, uint64_t* bsum, unsigned long long* total, hipStream_t st) {
  return sst_scan(v, n, bsum, total, st);
}
extern "C" int lsmk_sst_sizes(const lsmck_wal_cmd* ents, uint64_t n, uint64_t keys_bytes, uint64_t vals_bytes,
                              uint64_t* off, uint64_t* bsum, unsigned long long* info, hipStream_t st) {
  if (n) hipLaunchKernelGGL(sst_size, dim3(sst_grid(n)), dim3(256), 0, st, ents, n, keys_bytes, vals_bytes, off, info);
  return sst_scan(off, n, bsum, info + 1, st);
}
extern "C" int lsmk_sst_order(const lsmck_wal_cmd* ents, uint64_t n, const uint8_t* keys, uint64_t keys_bytes,
                              uint64_t vals_bytes, const uint64_t* tf, uint64_t ntab, uint8_t* first,
                              unsigned long long* info, hipStream_t st) {
  if (n < 2) return 0;
  hipLaunchKernelGGL(sst_first, dim3(sst_grid(ntab)), dim3(256), 0, st, tf, ntab, n, first);
  hipLaunchKernelGGL(sst_order, dim3(sst_grid(n - 1)), dim3(256), 0, st, ents, n, keys, keys_bytes, vals_bytes,
                     (const uint8_t*)first, info);
  return sst_launch_err();
}
extern "C" int lsmk_sst_index_plan(const uint32_t* item_ent, uint64_t nitems, const lsmck_wal_cmd* ents,
                                   uint64_t* ioff, uint64_t* bsum, unsigned long long* info, hipStream_t st) {
  if (nitems)
    hipLaunchKernelGGL(sst_index_size, dim3(sst_grid(nitems)), dim3(256), 0, st, item_ent, nitems, ents, ioff);
  return sst_scan(ioff, nitems, bsum, info + 3, st);
}
extern "C" int lsmk_sst_spans(const uint64_t* tf, const uint64_t* ibase, uint64_t ntab, const uint64_t* off,
                              const uint64_t* ioff, lsmck_sstable_span* spans, uint64_t* doff, uint32_t* dlen,
                              uint64_t* xoff, uint32_t* xlen, unsigned hash, unsigned long long* info,
                              hipStream_t st) {
  if (ntab == 0) return 0;
  hipLaunchKernelGGL(sst_spans, dim3(sst_grid(ntab)), dim3(256), 0, st, tf, ibase, ntab, off, ioff, spans, doff, dlen,
                     xoff, xlen, hash, info);
  return sst_launch_err();
}
extern "C" int lsmk_sst_gather(const uint8_t* keys, const uint8_t* vals, const lsmck_wal_cmd* ents, uint64_t n,
                               const uint64_t* off, uint8_t* img, uint64_t total, hipStream_t st) {
  if (n == 0 || total == 0) return 0;
  const uint64_t tiles = (((uintptr_t)img & (sst::kTile - 1u)) + total + sst::kTile - 1u) / sst::kTile;
  if (tiles > 0x7FFFFFFFull) return -(int)hipErrorInvalidValue;
  hipLaunchKernelGGL(sst_gather, dim3((unsigned)tiles), dim3(sst::kBlock), 0, st, keys, vals, ents, n, off, img);
  return sst_launch_err();
}
extern "C" int lsmk_sst_index_write(const uint32_t* item_tab, const uint32_t* item_ent, uint64_t nitems,
                                    const uint64_t* tf, const lsmck_wal_cmd* ents, const uint8_t* keys,
                                    const uint64_t* off, const uint64_t* ioff, uint8_t* index, hipStream_t st) {
  if (nitems == 0) return 0;
  hipLaunchKernelGGL(sst_index_write, dim3(sst_grid(nitems)), dim3(256), 0, st, item_tab, item_ent, nitems, tf, ents,
                     keys, off, ioff, index);
  return sst_launch_err();
}
