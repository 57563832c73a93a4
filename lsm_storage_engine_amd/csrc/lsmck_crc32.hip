// lsmck_crc32.hip -- batched CRC-32/ISO-HDLC ("checksum_ieee") for gfx950 (MI355X).
//
// Replaces, in bulk, the per-record `crc::crc32::checksum_ieee(&[u8]) -> u32`
// that the reference calls on every WAL record (src/wal.rs:135,153 on replay,
// :177,187 on append).  Bit-exact with crc 1.x: reflected poly 0xEDB88320,
// init 0xFFFFFFFF, xorout 0xFFFFFFFF.
//
// Design (DESIGN.md section 3 has the derivation and the measurements behind it):
//   * Every record is cut into 128-byte SEGMENTS aligned to the record's END;
//     only the record's first segment can be short, and it is front-padded with
//     zeros (leading zeros do not change a CRC whose register starts at 0).
//   * One lane owns one segment and streams it from HBM itself: lane-contiguous
//     128-B segments measured 6.42 TB/s on MI355X (tools/microbench.hip), better
//     than the wave-coalesced 16 B/lane pattern.  Loads are dword-aligned
//     dwordx4 (byte-misaligned vector loads measured 3x slower) and a
//     v_alignbyte funnel produces the byte stream; loads never touch a dword
//     that does not intersect the record (no over-read past either end).
//   * The lane runs a raw (init 0) slicing-by-4 CRC over its 32 words.  The four
//     256-entry tables live in LDS replicated 32x so that lane l only ever reads
//     bank l%32: conflict-free random lookups (17 lookups/clk/CU measured vs
//     9.8 for plain tables); the LDS byte address of entry e is
//     256*e + 4*(lane%32) (+128, +64 KiB for the other tables), formed by ONE
//     v_perm_b32 from the state word and a per-lane constant.
//   * Segment results are combined with the CRC combination law
//        raw(A||B) = raw(A) (x) x^(8|B|)  xor  raw(B)   (GF(2)[x] mod P)
//     Each lane multiplies by x^(8*128*k) (k = segments after it; table in HBM,
//     L2-resident), the record's first segment also folds in the init term
//     0xFFFFFFFF (x) x^(8*len0), and a segmented XOR across the wave's lanes
//     collects each record at its first lane.  Records entirely inside one
//     wave tile are stored directly; records spanning tiles XOR their partial
//     results into a zeroed output with atomics (XOR is order independent, so
//     the result is deterministic).
//   * Persistent grid: one 1024-thread workgroup per CU (the 128 KiB of tables
//     are built once per CU), 16 waves per CU, each wave walks 64-segment tiles.
#include <hip/hip_runtime.h>
#include <stdint.h>
#ifdef LSMCK_WAVE_DIAG
#include <stdio.h>
#include <stdlib.h>

#include <vector>
#endif

#include "lsmck_device.h"
#include "lsmck_splan.h"

namespace lsmck {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#define LDS_TABLE_BYTES 131072u  // slicing-by-4 tables, 32x bank-replicated
#define LDS_SHIFT_OFF 131072u    // chain-combine tables: shift by 32, 64, 96 bytes (3 x 4 x 256 x 4 B)
#define LDS_SHIFT_BYTES 12288u
#define LDS_COLS_OFF (LDS_SHIFT_OFF + LDS_SHIFT_BYTES)  // fixed records: per-lane columns of x^(8*128*k)
#define LDS_COLS_BYTES 8192u                               // [32/4][64 lanes][4] u32
#define LDS_KHI_OFF (LDS_COLS_OFF + LDS_COLS_BYTES)  // khi[0..511]: x^(8*128*65536*j), j = k >> 16 (len < 2^32)
#define LDS_KHI_BYTES 2048u
// per-segment factor K = x^(8*128*k) = klo[k & 511] (x) kmid[(k >> 9) & 127] (x) khi[k >> 16],
// and the init terms tinit[len0]: all from LDS, so the issue path gathers no tables
#define LDS_KLO_OFF (LDS_KHI_OFF + LDS_KHI_BYTES)
#define LDS_KMID_OFF (LDS_KLO_OFF + 2048u)
#define LDS_TINIT_OFF (LDS_KMID_OFF + 512u)
#define LDS_SCRATCH_OFF (LDS_TINIT_OFF + 544u)
#define WAVE_SCRATCH_BYTES 256u
// stream kernel: per wave 64 chunks x {end, start} x 2 chains, the chain byte
// + 1 (0 = none), written by the window lanes, read and cleared by the chunk lanes
#define LDS_SMAP_OFF LDS_SCRATCH_OFF
#define LDS_SMAP_BYTES 4096u
// ---------------------------------------------------------------------------
// GF(2) polynomial product modulo the reflected CRC-32 polynomial.
// Same function as zlib's multmodp; branch-free, 32 steps.
__device__ __forceinline__ uint32_t gf2_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    uint32_t m = (uint32_t)((int32_t)(a << i) >> 31);
    p ^= b & m;
    b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
  }
  return p;
}

// 128-byte segments of a non-empty record: ceil(len / 128) for every uint32_t
// len -- (len + 127) >> 7 wraps to 0 for the top 127 lengths (len > 2^32 - 128).
__host__ __device__ __forceinline__ uint32_t segs_of(uint32_t len) { return (len >> 7) + ((len & 127u) != 0u); }

// The kernels declare no static LDS, so the dynamic region starts at LDS
// address 0: index an address_space(3) pointer directly (indexing smem + a
// costs a v_add of the relocated base per lookup).
typedef __attribute__((address_space(3))) const uint32_t lds_u32_t;
typedef __attribute__((address_space(3))) const u32x4 lds_u32x4_t;
__device__ __forceinline__ uint32_t lds_ld(const unsigned char* smem, uint32_t a) {
  (void)smem;
  return *(lds_u32_t*)(size_t)a;
}
__device__ __forceinline__ u32x4 lds_ld128(uint32_t a) { return *(lds_u32x4_t*)(size_t)a; }

// ---------------------------------------------------------------------------
// LDS tables.  Byte address of T_t[e], replica r:
//   256*e + 4*r + 128*(t&1) + 65536*(t>>1)
// T0 = Sarwate table, T_k[n] = (T_{k-1}[n] >> 8) ^ T0[T_{k-1}[n] & 0xFF].
__device__ __forceinline__ void build_lds_tables(unsigned char* smem, const CrcParams& P) {
  const uint32_t* __restrict__ master = P.master;
  uint32_t* s32 = (uint32_t*)smem;
  for (uint32_t i = threadIdx.x; i < LDS_TABLE_BYTES / 4; i += blockDim.x) {
    uint32_t t = ((i >> 14) << 1) | ((i >> 5) & 1u);
    uint32_t e = (i >> 6) & 255u;
    s32[i] = master[t * 256u + e];
  }
  // shift tables ST_m[j][b] = (b << 8j) (x) x^(8*32m) mod P, m = 1..3, plain layout
  for (uint32_t i = threadIdx.x; i < LDS_SHIFT_BYTES / 4; i += blockDim.x) s32[LDS_SHIFT_OFF / 4 + i] = master[1024u + i];
  // segment factors of records over 2^16 segments (8 MiB): from LDS, so the
  // checksum loop issues no global load of its own (its waits would also
  // wait for the next tile's prefetch)
  for (uint32_t i = threadIdx.x; i < LDS_KHI_BYTES / 4; i += blockDim.x) s32[LDS_KHI_OFF / 4 + i] = P.khi[i];
  for (uint32_t i = threadIdx.x; i < 512u; i += blockDim.x) s32[LDS_KLO_OFF / 4 + i] = P.kseg[i];
  for (uint32_t i = threadIdx.x; i < 128u; i += blockDim.x) s32[LDS_KMID_OFF / 4 + i] = P.kseg[512u * i];
  for (uint32_t i = threadIdx.x; i < 130u; i += blockDim.x) s32[LDS_TINIT_OFF / 4 + i] = P.tinit[i];
}

// raw CRC register s advanced over 32*m zero bytes (m = 1..3): 4 plain-table lookups
template <int M>
__device__ __forceinline__ uint32_t shift_bytes32(const unsigned char* smem, uint32_t s) {
  constexpr uint32_t base = LDS_SHIFT_OFF + (M - 1) * 4096u;
  return lds_ld(smem, base + ((s & 0xFFu) << 2)) ^ lds_ld(smem, base + 1024u + (((s >> 8) & 0xFFu) << 2)) ^
         lds_ld(smem, base + 2048u + (((s >> 16) & 0xFFu) << 2)) ^ lds_ld(smem, base + 3072u + ((s >> 24) << 2));
}


// One slicing-by-4 step of the raw CRC register: s' = F(s ^ w).
// lo = lane4, hi = lane4 | 0x10000 (region of T2/T3).
__device__ __forceinline__ uint32_t crc_word(const unsigned char* smem, uint32_t s, uint32_t w, uint32_t lo,
                                             uint32_t hi) {
  uint32_t x = s ^ w;
  uint32_t a0 = __builtin_amdgcn_perm(x, hi, 0x0c020400u);  // byte0 -> T3
  uint32_t a1 = __builtin_amdgcn_perm(x, hi, 0x0c020500u);  // byte1 -> T2
  uint32_t a2 = __builtin_amdgcn_perm(x, lo, 0x0c0c0600u);  // byte2 -> T1
  uint32_t a3 = __builtin_amdgcn_perm(x, lo, 0x0c0c0700u);  // byte3 -> T0
  return lds_ld(smem, a0 + 128u) ^ lds_ld(smem, a1) ^ lds_ld(smem, a2 + 128u) ^ lds_ld(smem, a3);
}

// The same step on x = s ^ w already formed, folding in the NEXT word:
// returns F(x) ^ w_next, the next step's x, as two v_bitop3_b32 (xor3) --
// instead of three v_xor for F and one for the next s ^ w.
__device__ __forceinline__ uint32_t crc_step_x(const unsigned char* smem, uint32_t x, uint32_t w_next, uint32_t lo,
                                               uint32_t hi) {
  uint32_t a0 = __builtin_amdgcn_perm(x, hi, 0x0c020400u);  // byte0 -> T3
  uint32_t a1 = __builtin_amdgcn_perm(x, hi, 0x0c020500u);  // byte1 -> T2
  uint32_t a2 = __builtin_amdgcn_perm(x, lo, 0x0c0c0600u);  // byte2 -> T1
  uint32_t a3 = __builtin_amdgcn_perm(x, lo, 0x0c0c0700u);  // byte3 -> T0
  const uint32_t l2 = lds_ld(smem, a2 + 128u), l3 = lds_ld(smem, a3);
  const uint32_t t = __builtin_amdgcn_bitop3_b32(l2, l3, w_next, 0x96);
  return __builtin_amdgcn_bitop3_b32(lds_ld(smem, a0 + 128u), lds_ld(smem, a1), t, 0x96);
}

// The step on two chains at once, all eight lookups issued before the first
// XOR.  The stream kernel's event loop uses it: with its word bodies as
// branches the two crc_step_x calls came out one after the other, each
// waiting for its own lookups (two LDS round trips per word and chain).
__device__ __forceinline__ void crc_step_x2(uint32_t& c0, uint32_t& c1, uint32_t x0, uint32_t n0, uint32_t x1,
                                            uint32_t n1, uint32_t lo, uint32_t hi) {
  const uint32_t a00 = __builtin_amdgcn_perm(x0, hi, 0x0c020400u), a01 = __builtin_amdgcn_perm(x0, hi, 0x0c020500u);
  const uint32_t a02 = __builtin_amdgcn_perm(x0, lo, 0x0c0c0600u), a03 = __builtin_amdgcn_perm(x0, lo, 0x0c0c0700u);
  const uint32_t a10 = __builtin_amdgcn_perm(x1, hi, 0x0c020400u), a11 = __builtin_amdgcn_perm(x1, hi, 0x0c020500u);
  const uint32_t a12 = __builtin_amdgcn_perm(x1, lo, 0x0c0c0600u), a13 = __builtin_amdgcn_perm(x1, lo, 0x0c0c0700u);
  const uint32_t l02 = lds_ld(nullptr, a02 + 128u), l03 = lds_ld(nullptr, a03);
  const uint32_t l00 = lds_ld(nullptr, a00 + 128u), l01 = lds_ld(nullptr, a01);
  const uint32_t l12 = lds_ld(nullptr, a12 + 128u), l13 = lds_ld(nullptr, a13);
  const uint32_t l10 = lds_ld(nullptr, a10 + 128u), l11 = lds_ld(nullptr, a11);
  c0 = __builtin_amdgcn_bitop3_b32(l00, l01, __builtin_amdgcn_bitop3_b32(l02, l03, n0, 0x96), 0x96);
  c1 = __builtin_amdgcn_bitop3_b32(l10, l11, __builtin_amdgcn_bitop3_b32(l12, l13, n1, 0x96), 0x96);
}

// ---------------------------------------------------------------------------
// Segment loading.
//
// A segment's byte stream is the 128 bytes [E-128, E) (absolute addresses),
// of which only [B, E) are record bytes (B = E-128 except for a record's short
// first segment).  Dwords D_i live at base4 + 4i, base4 = floor4(E-128),
// i = 0..32; stream word j = alignbyte(D_{j+1}, D_j, (E-128)&3).
// Dword i is loaded only if it intersects [B, E): i >= lo_i, and D_32 only if
// (E-128) is not dword aligned.  Nothing outside the record's dwords is read.
__device__ __forceinline__ uint32_t ld32(const unsigned char* p) { return *(const uint32_t*)p; }
__device__ __forceinline__ u32x4 ld128(const unsigned char* p) { return *(const u32x4*)p; }

// Keep a load's address VGPRs live past the segment's loads.  Otherwise hipcc
// lets the last load of a segment write its data over the address register
// (e.g. `buffer_load_dwordx4 v[34:37], v34, ... offset:112`), and that form
// streams 14-20% slower on gfx950: tools/microbench_policy.hip measured 12.4
// vs 10.75 ms for 64 GB with the same addresses, and 13.0 vs 10.76 ms for
// eight per-load offsets whose registers the next tile's loads overwrite
// (profiles/r01/ablations.md, "Load instruction form").
template <typename T>
__device__ __forceinline__ void keep_live(const T& x) {
  asm volatile("" ::"v"(x));
}

struct SegInfo {
  uint32_t rec;       // record index
  uint32_t q;         // segment index from the record's front
  uint32_t k;         // segments after this one
  uint64_t rec_off;   // record offset from base
  uint32_t rec_len;
  bool valid;
};

// In-flight loads of one segment (issued one tile ahead of their use).
struct SegLoad {
  uint32_t d[33];  // dwords D_0..D_32 (D_32 only when the stream start is not dword aligned)
  // the segment's coordinates, copied at issue time (when they are resident):
  // finish needs no SegInfo, so the map of a later tile may still be in flight
  uint32_t rec, k;
  uint32_t fl;     // packed SegLoad.fl fields below
};
// FL_SH: (E-128) & 3.  FL_BST: B - floor4(E-128).  FL_VALID: lane holds a
// real segment.  FL_FIRST: q == 0.  FL_M: the load window was moved up by
// m dwords to the start of B's page (see seg_issue); seg_finish moves the
// registers back.
#define FL_SH(f) ((f) & 3u)
#define FL_BST(f) (((f) >> 2) & 0xFFu)
#define FL_VALID 0x400u
#define FL_FIRST 0x800u
#define FL_M(f) (((f) >> 12) & 0x3Fu)

// Issue every global load of a segment; consumes nothing.  FAST: full
// segment whose stream start is dword aligned.
template <bool FAST, int ABLATE = 0>
__device__ __forceinline__ void seg_issue(const CrcParams& P, const SegInfo& si, SegLoad& L) {
  const uint64_t E = si.rec_off + si.rec_len - 128ull * si.k;  // segment end (offset from base)
  const uint32_t seglen = (si.q == 0) ? si.rec_len - 128u * si.k : 128u;
  const uint32_t lead = 128u - seglen;  // stream bytes in front of the record (first segment only)
  L.rec = si.rec;
  L.k = si.k;
  const uint32_t flv = (si.valid ? FL_VALID : 0u) | (si.q == 0 ? FL_FIRST : 0u);
  L.fl = flv;
  // pointer arithmetic on the kernel-argument pointer keeps these global_load (not flat_load)
  const unsigned char* s0 = P.base + (E - 128);
  if (FAST) {
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      u32x4 v = ld128(s0 + 16 * g);
      L.d[4 * g + 0] = v.x;
      L.d[4 * g + 1] = v.y;
      L.d[4 * g + 2] = v.z;
      L.d[4 * g + 3] = v.w;
    }
    keep_live(s0);
    L.d[32] = 0;
    return;
  }
  // General path: one base pointer per lane, eight 16-byte loads at
  // immediate offsets (per-group addresses cost ~30% of the load path:
  // crc_ablate 3 vs 6), straight-line (a divergent branch here makes hipcc
  // wait for the loads and the prefetch is lost).
  //  - window [p, p+128), p = floor4(E-128): it never passes E.  Bytes of it
  //    in front of B (first segments) are zeroed in seg_finish;
  //  - they are on B's page unless a page boundary lies in (p, B].  A page
  //    boundary is dword aligned, so it can only fall in front of B's dword,
  //    never inside the stream of a non-first segment.  Then the window starts
  //    at the boundary instead (m = 1..32 dwords higher; it ends at most 131
  //    bytes into B's page) and seg_finish shifts the registers back up;
  //  - D_32 (stream bytes only when the stream start is not dword aligned)
  //    is the dword at p+128, which holds E-1 when it is needed; otherwise a
  //    dword inside the window is loaded and ignored;
  //  - an empty segment (empty record, pad lane) reads a zero buffer.
  const uint32_t sh = (uint32_t)((uintptr_t)s0 & 3);
  const unsigned char* p = s0 - sh;  // floor4(E-128)
  const uint32_t bstart = sh + lead; // B - p
  const bool empty = lead >= 128u;
  const uintptr_t pa = (uintptr_t)p;
  const uintptr_t pg = (pa + bstart) & ~(uintptr_t)4095;  // B's page
  const bool cross = !empty & (pg > pa);
  const uint32_t m = cross ? (uint32_t)(pg - pa) >> 2 : 0u;  // 1..32
  L.fl = flv | sh | (bstart << 2) | (m << 12);
  // pointer arithmetic from the kernel-argument pointers keeps these global_load
  const unsigned char* w = empty ? (const unsigned char*)P.zero : p + 4u * m;
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    u32x4 v = ld128(w + 16 * g);
    L.d[4 * g + 0] = v.x;
    L.d[4 * g + 1] = v.y;
    L.d[4 * g + 2] = v.z;
    L.d[4 * g + 3] = v.w;
  }
  L.d[32] = ld32(w + ((sh != 0u && m == 0u) ? 128 : 124));
  keep_live(w);
}

// Funnel, mask, raw slicing-by-4 CRC, init term, shift to the record's end.
// CHAINS independent register chains per lane (the segment's 128 bytes cut in
// CHAINS pieces) hide the LDS lookup latency; they are recombined with the
// shift-by-32m-bytes tables: raw(A||B) = shift_|B|(raw(A)) ^ raw(B).
template <bool FAST, int CHAINS, int ABLATE = 0, bool PERCOL = false, bool RAW = false>
__device__ __forceinline__ uint32_t seg_finish(const unsigned char* smem, const CrcParams& P, const SegLoad& L,
                                               uint32_t lo, uint32_t hi) {
  if (ABLATE == 3) {  // diagnostic: loads only (results invalid)
    uint32_t x = 0;
#pragma unroll
    for (int j = 0; j < 33; ++j) x ^= L.d[j];
    return x ^ L.k ^ L.fl;
  }
  uint32_t w[32];
  if (FAST) {
#pragma unroll
    for (int j = 0; j < 32; ++j) w[j] = L.d[j];
  } else {
    uint32_t d[33];
#pragma unroll
    for (int j = 0; j < 33; ++j) d[j] = L.d[j];
    const uint32_t sh = FL_SH(L.fl), bstart = FL_BST(L.fl), lo_i = bstart >> 2;
    const uint32_t bm = 0xFFFFFFFFu << (8u * (bstart & 3u));  // keep-mask of B's dword
    const uint32_t m = FL_M(L.fl);
    if (__any(m != 0u)) {  // rare: the window started at B's page, m dwords up: shift back
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        const int s = 1 << b;
        const bool on = (m >> b) & 1u;
#pragma unroll
        for (int j = 32; j >= 0; --j) d[j] = on ? (j >= s ? d[j - s] : 0u) : d[j];
      }
    }
    if (__any(bstart != 0u)) {
      // zero the window in front of B: the groups before B's group and the
      // bytes of B's group in front of B (with lead = 0 this only clears bytes
      // of D_0 in front of the stream start, which the funnel drops anyway)
      const uint32_t r = lo_i & 3u, gb = lo_i >> 2;
      uint32_t mk[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) mk[k] = ((uint32_t)k < r) ? 0u : (((uint32_t)k == r) ? bm : 0xFFFFFFFFu);
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const bool before = (uint32_t)g < gb, here = (uint32_t)g == gb;
#pragma unroll
        for (int k = 0; k < 4; ++k) d[4 * g + k] &= before ? 0u : (here ? mk[k] : 0xFFFFFFFFu);
      }
      d[32] &= (lo_i == 32u) ? bm : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int j = 0; j < 32; ++j) w[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], sh);
  }
  constexpr int WPC = 32 / CHAINS;  // words per chain
  // each chain carries x = state ^ (its next word); the state starts at 0, so
  // the first x is the first word, and the last step folds in 0
  uint32_t c[CHAINS];
#pragma unroll
  for (int h = 0; h < CHAINS; ++h) c[h] = w[h * WPC];
#pragma unroll
  for (int j = 0; j < WPC; ++j) {
#pragma unroll
    for (int h = 0; h < CHAINS; ++h) c[h] = crc_step_x(smem, c[h], j + 1 < WPC ? w[h * WPC + j + 1] : 0u, lo, hi);
  }
  uint32_t s;
  if constexpr (CHAINS == 1) {
    s = c[0];
  } else if constexpr (CHAINS == 2) {
    s = shift_bytes32<2>(smem, c[0]) ^ c[1];
  } else {
    s = shift_bytes32<3>(smem, c[0]) ^ shift_bytes32<2>(smem, c[1]) ^ shift_bytes32<1>(smem, c[2]) ^ c[3];
  }
  // init term of a record's first segment: 0xFFFFFFFF (x) x^(8*len0), len0 = 128 - lead
  const uint32_t lead0 = FL_BST(L.fl) - FL_SH(L.fl);
  s ^= (L.fl & FL_FIRST) ? lds_ld(smem, LDS_TINIT_OFF + ((128u - lead0) << 2)) : 0u;
  if constexpr (RAW) return s;  // walking kernel: shifted by the caller (Horner within the tile)
  if constexpr (PERCOL) {
    // s (x) K with the lane's 32 precomputed columns K*x^i: p ^= col_i if bit 31-i of s
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t p = 0;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      u32x4 c = lds_ld128(LDS_COLS_OFF + g * 1024u + lane * 16u);
      // p ^= col & mask as one v_bitop3_b32 (truth table 0x78: a ^ (b & c))
      p = __builtin_amdgcn_bitop3_b32(p, c.x, (uint32_t)((int32_t)(s << (4 * g + 0)) >> 31), 0x78);
      p = __builtin_amdgcn_bitop3_b32(p, c.y, (uint32_t)((int32_t)(s << (4 * g + 1)) >> 31), 0x78);
      p = __builtin_amdgcn_bitop3_b32(p, c.z, (uint32_t)((int32_t)(s << (4 * g + 2)) >> 31), 0x78);
      p = __builtin_amdgcn_bitop3_b32(p, c.w, (uint32_t)((int32_t)(s << (4 * g + 3)) >> 31), 0x78);
    }
    return p;
  }
  uint32_t K = lds_ld(smem, LDS_KLO_OFF + ((L.k & 511u) << 2));
  if (__any(L.k >= 512u)) {  // records over 64 KiB (identity factors for the other lanes)
    K = gf2_mulmod(K, lds_ld(smem, LDS_KMID_OFF + (((L.k >> 9) & 127u) << 2)));
    if (__any(L.k >= 65536u)) K = gf2_mulmod(K, lds_ld(smem, LDS_KHI_OFF + ((L.k >> 16) << 2)));
  }
  return gf2_mulmod(s, K);
}

// Per-lane columns K*x^i (i = 0..31) of the shift factor K = x^(8*128*k_lane)
// for fixed records whose segment count divides 64: every tile starts on a
// record boundary, so lane l always holds segment k = nsegr-1 - l%nsegr.
__device__ __forceinline__ void build_lds_cols(const CrcParams& P, uint32_t nsegr) {
  if (threadIdx.x >= 64) return;
  const uint32_t lane = threadIdx.x;
  uint32_t b = P.kseg[nsegr - 1u - lane % nsegr];
  uint32_t* s32 = (uint32_t*)0;
  (void)s32;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    *(__attribute__((address_space(3))) uint32_t*)(size_t)(LDS_COLS_OFF + (i >> 2) * 1024u + lane * 16u + (i & 3) * 4u) = b;
    b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
  }
}

// ---------------------------------------------------------------------------
// Segmented XOR over a wave, for record heads: XOR of lanes [lane, run_end]
// = X[run_end] ^ X[lane-1] with X the inclusive prefix XOR of the wave.  The
// prefix runs on the VALU through DPP (row_shr 1/2/4/8 inside each 16-lane
// row, then row_bcast 15/31 across rows); only the gather of X[run_end] uses
// the LDS crossbar (one ds_bpermute instead of six shuffles): the LDS pipe is
// the checksum's bottleneck, the VALU has room.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp0(uint32_t x) {  // lanes without a source (or masked rows) read 0
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ uint32_t wave_prefix_xor(uint32_t x) {
  x ^= dpp0<0x111, 0xF>(x);  // row_shr:1
  x ^= dpp0<0x112, 0xF>(x);  // row_shr:2
  x ^= dpp0<0x114, 0xF>(x);  // row_shr:4
  x ^= dpp0<0x118, 0xF>(x);  // row_shr:8
  x ^= dpp0<0x142, 0xA>(x);  // row_bcast:15 -> rows 1, 3
  x ^= dpp0<0x143, 0xC>(x);  // row_bcast:31 -> rows 2, 3
  return x;
}
__device__ __forceinline__ uint32_t run_xor(uint32_t v, uint32_t run_end) {
  const uint32_t X = wave_prefix_xor(v);
  const uint32_t Xe = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(run_end << 2), (int)X);
  return Xe ^ dpp0<0x138, 0xF>(X);  // wave_shr:1 -> X[lane-1], 0 for lane 0
}

__device__ __forceinline__ void emit_record(const CrcParams& P, uint32_t v, const SegLoad& L, uint32_t lane,
                                            bool head) {
  if (!(L.fl & FL_VALID) || !head) return;
  bool has_last = (lane + L.k) <= 63u;  // this tile holds the record's final segment
  if ((L.fl & FL_FIRST) && has_last) {
    P.out[L.rec] = ~v;
  } else {
    atomicXor(&P.out[L.rec], has_last ? ~v : v);
  }
}

template <bool FAST, int CHAINS, int ABLATE = 0, bool PERCOL = false>
__device__ __forceinline__ void finish_tile(const unsigned char* smem, const CrcParams& P, const SegLoad& L,
                                            uint32_t lane, uint32_t lo, uint32_t hi) {
  uint32_t v = seg_finish<FAST, CHAINS, ABLATE, PERCOL>(smem, P, L, lo, hi);
  if (ABLATE == 3) {  // no reduction, no store (unless a magic value: keeps the loads alive)
    if (v == 0x9E3779B1u) P.out[0] = v;
    return;
  }
  v = (L.fl & FL_VALID) ? v : 0u;
  v = run_xor(v, min(63u, lane + L.k));
  emit_record(P, v, L, lane, lane == 0 || (L.fl & FL_FIRST));
}

// ---------------------------------------------------------------------------
// Fixed-size records: record r = [r*stride, r*stride + len).
__device__ __forceinline__ SegInfo fixed_map(const CrcParams& P, uint32_t t, uint32_t lane, uint32_t nsegr,
                                             uint32_t total) {
  uint32_t g = t * 64u + lane;
  SegInfo si;
  si.valid = g < total;
  uint32_t gg = si.valid ? g : total - 1u;
  si.rec = gg / nsegr;
  si.q = gg - si.rec * nsegr;
  si.k = nsegr - 1u - si.q;
  si.rec_off = (uint64_t)si.rec * P.stride;
  si.rec_len = P.flen;
  return si;
}

// Software pipelined: the loads of tile t+nwaves are in flight while tile t is
// checksummed (sched_barrier keeps the compiler from sinking them to their use).
// The layouts the ring kernel below does not take: records that are not
// dword aligned or whose segment count does not divide 64.
template <bool FAST, int CHAINS, int ABLATE = 0, bool PERCOL = false>
__global__ __launch_bounds__(1024) void crc32_fixed_kernel(CrcParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  build_lds_tables(smem, P);
  if (PERCOL) build_lds_cols(P, segs_of(P.flen));
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t lo = (lane & 31u) * 4u, hi = lo | 0x10000u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);  // uniform: scalar loop control
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  const uint32_t nsegr = segs_of(P.flen);
  const uint32_t total = nsegr * (uint32_t)P.nrec;  // host keeps this < 2^32 - 64
  const uint32_t ntiles = (total + 63u) >> 6;
  // ping-pong between two load slots A/B: a loaded register is never copied
  // (a copy would force s_waitcnt vmcnt(0) on the prefetch).  The loop has one
  // exit, at the bottom, with a precomputed trip count: a break between the
  // halves gives the CFG a second path into the header on which the other
  // slot's loads are still outstanding, and the wait-count merge then waits
  // for the prefetch at the top of every iteration.
  const uint32_t t0 = wave;
  if (t0 >= ntiles) return;
  const uint32_t niter = (ntiles - t0 + nwaves - 1u) / nwaves;  // tiles of this wave, >= 1
  uint32_t t = t0;
  SegLoad A, B;
  seg_issue<FAST, ABLATE>(P, fixed_map(P, t, lane, nsegr, total), A);
  for (uint32_t j = 2; j <= niter; j += 2) {
    const uint32_t tb = t + nwaves;
    seg_issue<FAST, ABLATE>(P, fixed_map(P, tb, lane, nsegr, total), B);
    __builtin_amdgcn_sched_barrier(0);
    finish_tile<FAST, CHAINS, ABLATE, PERCOL>(smem, P, A, lane, lo, hi);
    const uint32_t ta = (t + 2u * nwaves < ntiles) ? t + 2u * nwaves : t;  // past the end: reload, unused
    seg_issue<FAST, ABLATE>(P, fixed_map(P, ta, lane, nsegr, total), A);
    __builtin_amdgcn_sched_barrier(0);
    finish_tile<FAST, CHAINS, ABLATE, PERCOL>(smem, P, B, lane, lo, hi);
    t += 2u * nwaves;
  }
  if (niter & 1u) finish_tile<FAST, CHAINS, ABLATE, PERCOL>(smem, P, A, lane, lo, hi);
}

// ---------------------------------------------------------------------------
// Whole-tile ring (fixed records whose segment count divides 64, dword
// aligned: configs 1, 2 and 4): R slots of a whole tile, R-1 tiles in flight
// while one is checksummed.  Every tile starts on a record boundary, so a
// lane's byte offset from its tile's first record, (lane/nsegr)*stride +
// 128*(lane%nsegr), is the same in every tile: one offset VGPR per lane, the
// eight loads at immediate offsets from a wave-uniform buffer base, the
// register kept live past them (keep_live).  Each wave walks one contiguous
// range of tiles, so its records are consecutive: the CRCs are queued in one
// VGPR (lane p: record qb + p) and stored as whole 256-byte blocks, pushed
// after the next tile's loads are issued (profiles/r02/q: a per-tile store of
// a tile's two 4 KiB records cost 0.68 of 11.96 ms on config 2 and 0.94 GB of
// fetches per launch; a store or push between a tile's checksum and the next
// issue cost 1.2-1.5 ms whatever its address).  Pad lanes of the last tile
// fall past the batch's end: the buffer range returns zeros for them.
struct PercolMap {
  uint32_t lsh;      // log2(nsegr)
  uint64_t tstride;  // bytes per tile (64/nsegr records)
  uint64_t end;      // bytes from P.base to the last record's end
};
__device__ __forceinline__ void issue_whole(const CrcParams& P, const PercolMap& M, uint32_t vo, uint32_t t,
                                            uint32_t lane, uint32_t nsegr, uint32_t total, SegLoad& L) {
  const uint64_t tb = (uint64_t)t * M.tstride;
  const uint64_t left = M.end - tb;
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(P.base + tb), (short)0, (int)(left < 0x7FFFFFFFull ? left : 0x7FFFFFFFull), 0x00020000);
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    auto v = __builtin_amdgcn_raw_buffer_load_b128(r, vo + 16u * g, 0, 0);
    L.d[4 * g + 0] = v[0];
    L.d[4 * g + 1] = v[1];
    L.d[4 * g + 2] = v[2];
    L.d[4 * g + 3] = v[3];
  }
  keep_live(vo);
  L.d[32] = 0;
  const uint32_t gi = t * 64u + lane;
  const uint32_t q = gi & (nsegr - 1u);
  L.rec = gi >> M.lsh;
  L.k = nsegr - 1u - q;
  L.fl = (gi < total ? FL_VALID : 0u) | (q == 0u ? FL_FIRST : 0u);
}
template <int R, int ABLATE = 0>
__global__ __launch_bounds__(1024) void crc32_wring_kernel(CrcParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t nsegr = P.flen >> 7;
  build_lds_tables(smem, P);
  build_lds_cols(P, nsegr);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t lo = (lane & 31u) * 4u, hi = lo | 0x10000u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  const uint32_t total = nsegr * (uint32_t)P.nrec;
  const uint32_t ntiles = (total + 63u) >> 6;
  PercolMap M;
  M.lsh = __builtin_ctz(nsegr);
  M.tstride = (uint64_t)(64u >> M.lsh) * P.stride;
  M.end = (uint64_t)(P.nrec - 1) * P.stride + P.flen;
  const uint32_t vo = (uint32_t)((lane >> M.lsh) * P.stride) + 128u * (lane & (nsegr - 1u));
  const uint32_t m = 64u >> M.lsh;  // records per tile
  // this wave's tiles [t0, t0 + mine)
  const uint32_t per = (ntiles + nwaves - 1u) / nwaves, t0 = wave * per;
  if (t0 >= ntiles) return;
  const uint32_t mine = min(per, ntiles - t0);
  uint64_t qb = ((uint64_t)t0 * m) & ~63ull;
  uint32_t qv = 0, qs = (uint32_t)(((uint64_t)t0 * m) & 63u), qf = qs;
  auto qstore = [&](bool on) {
    const __amdgpu_buffer_rsrc_t r =
        __builtin_amdgcn_make_buffer_rsrc((void*)(P.out + qb), (short)0, 256, 0x00020000);
    if (on) __builtin_amdgcn_raw_buffer_store_b32(qv, r, lane << 2, 0, 0);
  };
  // the tile's records (head lanes 0, nsegr, ...; cnt of them valid) onto the queue
  auto qpush = [&](uint32_t v, uint32_t cnt) {
    const uint32_t k = (lane - qf) & 63u;  // the queue lane's record within the tile
    const uint32_t val = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((k << M.lsh) & 63u) << 2), (int)v);
    const uint32_t end = qf + cnt;  // cnt <= 64: at most one block completes
    qv = (lane >= qf && lane < end) ? val : qv;
    if (end >= 64u) {
      qstore(lane >= qs);
      qb += 64u;
      qs = 0u;
      qf = end - 64u;
      qv = lane < qf ? val : qv;
    } else {
      qf = end;
    }
  };
  const uint32_t iters = (mine + R - 1u) / R;
  // slots past the run's last tile reload its first tile (in bounds) and are
  // marked invalid (no store)
  auto tile_of = [&](uint32_t i) -> uint32_t { return i < mine ? t0 + i : t0; };
  SegLoad S[R];
  uint32_t dv = 0, dcnt = 0;  // the previous tile's CRCs, pushed after the next tile's loads are issued
#pragma unroll
  for (int k = 0; k < R - 1; ++k) {
    issue_whole(P, M, vo, tile_of(k), lane, nsegr, (k < (int)mine) ? total : 0u, S[k]);
    __builtin_amdgcn_sched_barrier(0);
  }
  uint32_t n0 = 0;
  for (uint32_t it = 0; it < iters; ++it) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const uint32_t ni = n0 + k + R - 1;
      issue_whole(P, M, vo, tile_of(ni), lane, nsegr, ni < mine ? total : 0u, S[(k + R - 1) % R]);
      __builtin_amdgcn_sched_barrier(0);
      if (dcnt) qpush(dv, dcnt);
      const uint32_t ti = n0 + k;  // this slot's tile, valid if ti < mine
      uint32_t v = seg_finish<true, 2, ABLATE, true>(smem, P, S[k % R], lo, hi);
      if (ABLATE == 3) {  // loads only: no reduction, no store (unless a magic value: keeps the loads alive)
        if (v == 0x9E3779B1u) P.out[0] = v;
        continue;
      }
      v = (S[k % R].fl & FL_VALID) ? v : 0u;
      dv = ~run_xor(v, min(63u, lane + S[k % R].k));
      const uint64_t r0 = (uint64_t)(t0 + ti) * m;  // the tile's first record
      dcnt = ti < mine ? (uint32_t)min((uint64_t)m, (uint64_t)P.nrec - r0) : 0u;
    }
    n0 += R;
  }
  if (ABLATE == 3) return;
  if (dcnt) qpush(dv, dcnt);
  qstore(lane >= qs && lane < qf);
}

// a walking-kernel lane's segment: segments after it; pad lanes (past the
// run's last segment) become empty first segments (they load only the zero
// buffer and store nothing)
__device__ __forceinline__ void desc_map_complete(SegInfo& si) {
  const uint32_t nseg = si.rec_len ? segs_of(si.rec_len) : 1u;
  si.k = nseg - 1u - si.q;
  if (!si.valid) {
    si.q = 0;
    si.k = 0;
    si.rec_len = 0;
  }
}

// ---------------------------------------------------------------------------
// Prep of the walking kernel: every record owns nseg = max(1, ceil(len/128))
// consecutive segments; walk_phase1 reduces nseg per WALK_SB-record
// superblock (four records per thread, one 16-byte load) and scan_phase2
// scans the superblock sums in u64.
__device__ __forceinline__ uint32_t rec_nseg(uint32_t len) { return len ? segs_of(len) : 1u; }

// the thread's four lengths (records >= n read as "absent": own = false)
__device__ __forceinline__ void load_len4(const uint32_t* __restrict__ len, uint64_t n, uint64_t r0, uint32_t l[4]) {
  if (r0 + 3 < n) {
    u32x4 v = *(const u32x4*)(len + r0);  // dword-aligned 16-byte load
    l[0] = v.x;
    l[1] = v.y;
    l[2] = v.z;
    l[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) l[j] = (r0 + j < n) ? len[r0 + j] : 0u;
  }
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dppv(int old, int x) {
  return __builtin_amdgcn_update_dpp(old, x, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ uint32_t wave_prefix_add(uint32_t x) {  // inclusive
  x += (uint32_t)dppv<0x111, 0xF>(0, (int)x);
  x += (uint32_t)dppv<0x112, 0xF>(0, (int)x);
  x += (uint32_t)dppv<0x114, 0xF>(0, (int)x);
  x += (uint32_t)dppv<0x118, 0xF>(0, (int)x);
  x += (uint32_t)dppv<0x142, 0xA>(0, (int)x);
  x += (uint32_t)dppv<0x143, 0xC>(0, (int)x);
  return x;
}
__device__ __forceinline__ int wave_prefix_max(int x) {  // inclusive, identity -1
  x = max(x, dppv<0x111, 0xF>(-1, x));
  x = max(x, dppv<0x112, 0xF>(-1, x));
  x = max(x, dppv<0x114, 0xF>(-1, x));
  x = max(x, dppv<0x118, 0xF>(-1, x));
  x = max(x, dppv<0x142, 0xA>(-1, x));
  x = max(x, dppv<0x143, 0xC>(-1, x));
  return x;
}

// single workgroup: exclusive scan of the block sums in place, total in *total.
// Thread i owns the contiguous chunk [i*C, (i+1)*C).
// skip: the stream kernel's flag -- set when it took the batch, so the walking
// kernel's segment prefix is not needed (nullptr: always run)
__global__ __launch_bounds__(1024) void scan_phase2(uint64_t* __restrict__ block_sum, uint32_t nblocks,
                                                     uint64_t* __restrict__ total, const uint32_t* skip = nullptr) {
  if (skip && *skip) return;
  __shared__ uint64_t wsum[16];
  const uint32_t C = (nblocks + 1023u) / 1024u;
  const uint32_t b0 = threadIdx.x * C, b1 = min(nblocks, b0 + C);
  uint64_t mine = 0;
  for (uint32_t b = b0; b < b1; ++b) mine += block_sum[b];
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t x = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint64_t o = __shfl_up(x, d, 64);
    if (lane >= (uint32_t)d) x += o;
  }
  if (lane == 63u) wsum[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t acc = 0;
    for (int i = 0; i < 16; ++i) {
      uint64_t v = wsum[i];
      wsum[i] = acc;
      acc += v;
    }
    *total = acc;
  }
  __syncthreads();
  uint64_t run = wsum[threadIdx.x >> 6] + x - mine;  // exclusive prefix of this chunk
  for (uint32_t b = b0; b < b1; ++b) {
    uint64_t v = block_sum[b];
    block_sum[b] = run;
    run += v;
  }
}

// ===========================================================================
// Walking descriptor kernel (the default for descriptor batches).
//
// Every wave owns ONE contiguous run of records -- whole superblocks of
// WALK_SB records, cut so that every wave gets about the same number of
// 128-byte segments (walk_phase1 + scan_phase2 give the segment prefix per
// superblock; a wave binary-searches its cut points) -- and walks the run's
// segments in order, 64 per tile.  So:
//  * no record is split between waves: every CRC is stored once, with a plain
//    store (no zeroing of `out`, no atomics);
//  * a record spanning tiles carries its partial value to the next tile in a
//    wave-uniform register (Horner: carry (x) x^(8*128*m) ^ the next tile's
//    part), so a lane only shifts its segment to the record's last lane IN THE
//    TILE, d < 64 segments: 32 precomputed LDS columns per d (8 ds_read_b128 +
//    32 v_bitop3) instead of the 32-step generic GF(2) multiply;
//  * the segment -> record map comes from windows of 64 records (one per lane:
//    off, len, prefix of segment counts) held in registers, three windows deep
//    (current, next, prefetched): no per-tile map in HBM.  The only scratch is
//    one u64 per superblock, sized by the record count, so the host never has
//    to read a device total back to size anything: the batch is asynchronous
//    on its stream;
//  * contiguous per-wave runs stream as fast as the strided tile order of the
//    fixed kernels (tools/microbench_walk.hip: 6.56 against 6.42 TB/s over
//    96 GiB, profiles/r02/mb/mb_walk96.log).
#define WALK_SB 256u
#define LDS_WCOLS_OFF LDS_COLS_OFF  // [8 groups][65 d][4 u32] columns of x^(8*128*d), d = 0..64 (8320 B)

// a wave per superblock, grid-strided over a grid of a few waves per CU (a
// batch the stream kernel took costs one small launch that exits at once)
__global__ __launch_bounds__(1024) void walk_phase1(const uint32_t* __restrict__ len, uint64_t n,
                                                     uint64_t* __restrict__ sb_sum, const uint32_t* skip) {
  if (skip && *skip) return;  // the stream kernel took the batch
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nsb = (n + WALK_SB - 1u) / WALK_SB;
  for (uint64_t sb = (uint64_t)blockIdx.x * 16u + (threadIdx.x >> 6); sb < nsb; sb += (uint64_t)gridDim.x * 16u) {
    const uint64_t r0 = sb * WALK_SB + lane * 4u;
    uint32_t l[4];
    load_len4(len, n, r0, l);
    uint64_t x = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) x += (r0 + j < n) ? rec_nseg(l[j]) : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    if (lane == 0) sb_sum[sb] = x;
  }
}

// columns K*x^i (i = 0..31) of K = x^(8*128*d), d = 0..64, for the Horner shifts
__device__ __forceinline__ void build_walk_cols(const CrcParams& P) {
  if (threadIdx.x > 64) return;
  const uint32_t d = threadIdx.x;
  uint32_t b = P.kseg[d];
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    *(__attribute__((address_space(3))) uint32_t*)(size_t)(LDS_WCOLS_OFF + ((i >> 2) * 65u + d) * 16u + (i & 3) * 4u) = b;
    b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
  }
}

// v (x) x^(8*128*d), d = 0..64, from the LDS columns
__device__ __forceinline__ uint32_t walk_mulcol(uint32_t v, uint32_t d) {
  uint32_t p = 0;
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const u32x4 c = lds_ld128(LDS_WCOLS_OFF + (g * 65u + d) * 16u);
    p = __builtin_amdgcn_bitop3_b32(p, c.x, (uint32_t)((int32_t)(v << (4 * g + 0)) >> 31), 0x78);
    p = __builtin_amdgcn_bitop3_b32(p, c.y, (uint32_t)((int32_t)(v << (4 * g + 1)) >> 31), 0x78);
    p = __builtin_amdgcn_bitop3_b32(p, c.z, (uint32_t)((int32_t)(v << (4 * g + 2)) >> 31), 0x78);
    p = __builtin_amdgcn_bitop3_b32(p, c.w, (uint32_t)((int32_t)(v << (4 * g + 3)) >> 31), 0x78);
  }
  return p;
}

// the same for a wave-uniform v and d = 1..64, spread over the lanes: lane i
// < 32 contributes column i if bit 31-i of v is set; XOR over lanes 0..31
__device__ __forceinline__ uint32_t walk_mulcol_uniform(uint32_t v, uint32_t d, uint32_t lane) {
  const uint32_t i = lane & 31u;
  const uint32_t col = lds_ld(nullptr, LDS_WCOLS_OFF + ((i >> 2) * 65u + d) * 16u + (i & 3u) * 4u);
  const uint32_t t = (lane < 32u && ((v >> (31u - i)) & 1u)) ? col : 0u;
  return (uint32_t)__builtin_amdgcn_readlane((int)wave_prefix_xor(t), 31);
}

__device__ __forceinline__ uint32_t wave_or_u32(uint32_t x) {  // OR over the wave (uniform)
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// a window: records w0 + lane of the run (lane-held), absent past the run's end
struct WalkWin {
  uint64_t off;
  uint32_t len;
  uint32_t p;    // exclusive prefix of the segment counts inside the window
  uint32_t ok;   // the record exists (in the run)
};
__device__ __forceinline__ void walk_win_issue(const CrcParams& P, uint64_t w0, uint64_t r1, uint32_t lane, WalkWin& W) {
  const uint64_t r = w0 + lane;
  W.ok = r < r1;
  const uint64_t rr = W.ok ? r : (r1 - 1u);  // r1 > 0 whenever a window is loaded
  W.off = P.off[rr];
  W.len = P.len[rr];
}
// segment prefix of a landed window; returns the window's segment total (uniform)
__device__ __forceinline__ uint32_t walk_win_scan(WalkWin& W) {
  const uint32_t ns = W.ok ? rec_nseg(W.len) : 0u;
  const uint32_t inc = wave_prefix_add(ns);
  W.p = inc - ns;
  return (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
}
__device__ __forceinline__ uint64_t start_bit(const WalkWin& W, int64_t rel) {
  // rel = position of the window's first segment relative to the tile start
  const int64_t s = rel + (int64_t)W.p;
  return (W.ok && s >= 1 && s <= 63) ? (1ull << s) : 0ull;
}

template <int CHAINS, int ABLATE = 0>
__global__ __launch_bounds__(1024) void crc32_walk_kernel(CrcParams P) {
  if (P.sflag && *P.sflag) return;  // crc32_stream_kernel took the batch
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  build_lds_tables(smem, P);
  __syncthreads();  // the column table reuses the khi/klo area the table build fills
  build_walk_cols(P);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t lo = (lane & 31u) * 4u, hi = lo | 0x10000u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const uint32_t nw = (gridDim.x * blockDim.x) >> 6;
  const uint64_t n = P.nrec;
  const uint64_t nsb = (n + WALK_SB - 1u) / WALK_SB;
  const uint64_t S = *P.total_segs;
  // this wave's superblocks [b0, b1): the first superblock whose segment
  // prefix reaches S*w/nw (lower bound), for w and w+1
  auto cut = [&](uint32_t w) -> uint64_t {
    if (w >= nw) return nsb;
    const uint64_t target = (S / nw) * w + (S % nw) * w / nw;  // floor(S*w/nw) without overflow
    uint64_t a = 0, b = nsb;
    while (a < b) {
      const uint64_t m = (a + b) >> 1;
      if (P.sb_prefix[m] < target) a = m + 1; else b = m;
    }
    return a;
  };
  const uint64_t b0 = cut(wave), b1 = cut(wave + 1);
  if (b0 >= b1) return;
  const uint64_t r0 = b0 * WALK_SB, r1 = min(n, b1 * WALK_SB);
  const uint64_t segs = (b1 < nsb ? P.sb_prefix[b1] : S) - P.sb_prefix[b0];
  const uint64_t ntile = (segs + 63u) >> 6;
  // windows: records [r0 + 64*wc, +64) (cur), the next (nxt), the one after (pre, in flight)
  WalkWin cur, nxt, pre;
  walk_win_issue(P, r0, r1, lane, cur);
  walk_win_issue(P, r0 + 64u, r1, lane, nxt);
  walk_win_issue(P, r0 + 128u, r1, lane, pre);
  uint64_t wc0 = r0;                      // first record of cur
  uint64_t Bc = 0;                         // run segment of cur's first segment
  const uint32_t totc0 = walk_win_scan(cur);
  uint64_t Bn = Bc + totc0;                // run segment of nxt's first segment
  uint32_t totn = walk_win_scan(nxt);
  uint64_t G = 0;                          // run segment at lane 0 of the tile being mapped
  uint64_t rg = r0;                        // record holding segment G
  uint32_t qg = 0;                         //   and its segment index there
  uint32_t carry = 0;                      // partial value of the record continuing across tiles
  SegLoad A, B;
  A.fl = 0;  // virtual tile before the first: no valid lane, nothing stored
  A.k = 0;
  A.rec = 0;

  // map the tile at G onto (record, segment) per lane, advance the cursor and the windows
  auto map_tile = [&]() -> SegInfo {
    const uint64_t m = start_bit(cur, (int64_t)(Bc - G)) | start_bit(nxt, (int64_t)(Bn - G));
    const uint64_t M = (uint64_t)wave_or_u32((uint32_t)m) | ((uint64_t)wave_or_u32((uint32_t)(m >> 32)) << 32);
    const uint64_t below = M & ((lane == 63u) ? ~0ull : ((2ull << lane) - 1ull));
    SegInfo si;
    const uint64_t rec = rg + (uint64_t)__builtin_popcountll(below);
    si.q = below ? lane - (63u - (uint32_t)__builtin_clzll(below)) : qg + lane;
    // pad lanes: past the run's last segment (no start bit marks the end of
    // the run's last record, so the record index alone cannot tell)
    si.valid = G + lane < segs;
    const uint32_t idx = (uint32_t)(si.valid ? rec - wc0 : 0u);  // < 128
    const int src = (int)((idx & 63u) << 2);
    const uint32_t ol_c = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)cur.off);
    const uint32_t oh_c = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)(cur.off >> 32));
    const uint32_t ln_c = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)cur.len);
    const uint32_t ol_n = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)nxt.off);
    const uint32_t oh_n = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)(nxt.off >> 32));
    const uint32_t ln_n = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)nxt.len);
    const bool in_c = idx < 64u;
    si.rec = (uint32_t)rec;
    si.rec_off = in_c ? (((uint64_t)oh_c << 32) | ol_c) : (((uint64_t)oh_n << 32) | ol_n);
    si.rec_len = in_c ? ln_c : ln_n;
    si.k = 0;
    // (defensive: a lane never addresses a segment its record does not have)
    si.valid = si.valid && si.q < (si.rec_len ? segs_of(si.rec_len) : 1u);
    desc_map_complete(si);  // k; pad lanes become empty first segments
    // cursor for the next tile: the record holding segment G + 64
    const uint32_t rec63 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(rec - wc0), 63);
    const uint32_t q63 = (uint32_t)__builtin_amdgcn_readlane((int)si.q, 63);
    const uint32_t k63 = (uint32_t)__builtin_amdgcn_readlane((int)si.k, 63);
    rg = wc0 + rec63 + (k63 ? 0u : 1u);
    qg = k63 ? q63 + 1u : 0u;
    G += 64u;
    // one window step when the cursor left cur (at most one per tile: a full
    // window holds >= 64 segments); branch-free, pre is reloaded every tile
    const bool rot = rg >= wc0 + 64u;
    cur.off = rot ? nxt.off : cur.off;
    cur.len = rot ? nxt.len : cur.len;
    cur.p = rot ? nxt.p : cur.p;
    cur.ok = rot ? nxt.ok : cur.ok;
    nxt.off = rot ? pre.off : nxt.off;
    nxt.len = rot ? pre.len : nxt.len;
    nxt.ok = rot ? pre.ok : nxt.ok;
    wc0 = rot ? wc0 + 64u : wc0;
    Bc = rot ? Bn : Bc;
    const uint32_t tn = walk_win_scan(nxt);
    Bn = Bc + (rot ? totn : (Bn - Bc));
    totn = tn;
    walk_win_issue(P, wc0 + 128u, r1, lane, pre);
    return si;
  };

  auto finish = [&](const SegLoad& L) {
    if (!__builtin_amdgcn_readfirstlane((int)(L.fl & FL_VALID))) return;  // virtual tile (lane 0 valid otherwise)
    uint32_t v = seg_finish<false, CHAINS, ABLATE, false, true>(smem, P, L, lo, hi);
    if (ABLATE == 3) {  // loads only (no reduction or store, unless a magic value keeps the loads alive)
      if (v == 0x9E3779B1u) P.out[0] = v;
      return;
    }
    const bool valid = (L.fl & FL_VALID) != 0;
    v = valid ? v : 0u;
    const uint32_t d = min(63u - lane, L.k);
    v = walk_mulcol(v, d);
    const uint32_t run_end = min(63u, lane + L.k);
    const uint32_t X = wave_prefix_xor(v);
    const uint32_t Xe = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(run_end << 2), (int)X);
    uint32_t total = Xe ^ dpp0<0x138, 0xF>(X);  // lanes [lane, run_end]
    const bool head = valid && (lane == 0u || (L.fl & FL_FIRST));
    // lane 0 continuing a record from the previous tile: Horner step
    const bool cont0 = !__builtin_amdgcn_readfirstlane((int)(L.fl & FL_FIRST));
    const uint32_t re0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)run_end);
    const uint32_t cm = cont0 ? walk_mulcol_uniform(carry, re0 + 1u, lane) : 0u;
    total ^= (lane == 0u) ? cm : 0u;
    const bool ends = head && (lane + L.k <= 63u);
    if (ends) P.out[L.rec] = ~total;
    const uint64_t cb = __ballot(head && lane + L.k > 63u);
    carry = cb ? (uint32_t)__builtin_amdgcn_readlane((int)total, __builtin_ctzll(cb)) : 0u;
  };

  // half-steps: map + issue tile t, then finish tile t-1; one bottom exit with
  // a precomputed trip count (see crc32_fixed_kernel)
  uint64_t t = 0;
  for (; t + 2 <= ntile; t += 2) {
    seg_issue<false, ABLATE>(P, map_tile(), B);
    __builtin_amdgcn_sched_barrier(0);
    finish(A);
    seg_issue<false, ABLATE>(P, map_tile(), A);
    __builtin_amdgcn_sched_barrier(0);
    finish(B);
  }
  if (t < ntile) {
    seg_issue<false, ABLATE>(P, map_tile(), B);
    __builtin_amdgcn_sched_barrier(0);
    finish(A);
    finish(B);
  } else {
    finish(A);
  }
}

// ===========================================================================
// Stream kernel: a batch of records that are sorted and do not overlap --
// packed back to back (config 3), or with gaps between them (a WAL image: the
// 13- or 9-byte record header between two payloads, wal.rs:165-196).  The
// lanes read the batch as ALIGNED 128-byte chunks of the byte stream, the
// fixed ring kernel's load shape (buffer loads from a wave-uniform tile base,
// no per-lane address from the descriptors: tools/microbench_c3.hip, 16.2
// against 18.2 ms for config 3's per-record segment windows).  Record starts
// are CRC register resets and record ends are captures, so the bytes between
// records are read and dropped.  tools/stream_sim.py is the lane-level model
// of the algebra below, checked against zlib:
//  * a chunk is 32 words in two chains of 16.  A LONG record (>= 64 bytes)
//    has a start and an end event; a chain holds at most one end and one
//    start, the end first.  At a start at chunk byte j the chain's register
//    after the word is reset to F(~(u | mlo)) ^ mlo (the new record's bytes
//    from j, init folded in); at an end the capture A' = the register
//    advanced over the word's bytes before j (slicing-by-t, after the chains);
//  * the chunk's tail T (the last piece, aligned to the chunk end) is carried
//    Horner-wise to the chunk before the next END chunk: T (x) x^(1024 d)
//    from the LDS columns, a prefix XOR X over the wave, a wave-uniform carry
//    across tiles (entering lane 0's chain 0 as its initial register);
//  * a record ending at byte j of chunk c, started at chunk s of this tile:
//    CRC = ~(P (x) x^(8m) ^ A'), P = H (chain 0) or shift64(H) ^ R0 (chain
//    1), H = Y(c) ^ Y(s), Y(c) = X[c-1], m = j - 64h -- computed by the
//    window lane that holds the record, so every CRC is one plain, coalesced
//    store;
//  * a SHORT record (< 64 bytes: two of its events could share a chain) has
//    no events: its window lane checksums its bytes directly.
// The window: records bt + lane (off, len), loaded one tile ahead and slid by
// the count of records that end in the tile (ds_bpermute; only the new
// entries are loaded).  A tile in which all 64 window records end walks the
// next 64 too.  Slice s holds the records [scuts[s], scuts[s+1]) (stream_cuts:
// balanced by bytes) and the tiles that hold them; a wave takes slice after
// slice (one per wave on a small batch).  The first tile of a slice
// starts at its first record's start (the bytes in front are dropped).
// Eligibility: every batch the library builds itself (host-staged chunks, WAL
// replay) is sorted by construction and its gaps lie inside one buffer; a
// caller's device batch is checked on the device first (stream_check) and
// the walking kernel, launched after this one, takes it when it is not.
#define STREAM_LONG 64u      // records of at least this many bytes go through the chains
#define STREAM_MAX_GAP 64u   // caller batches: at most this many bytes between two records
// LDS columns K (x) x^i, i = 0..31 (128 B per factor K) of the finish
// factors x^(8m): m = 0..31 over the shift-by-32-bytes table,
// m = 32..63 over the shift-by-96-bytes table (only shift-by-64 is used here)
#define LDS_XMC_OFF(m) ((m) < 32u ? LDS_SHIFT_OFF + (m) * 128u : LDS_SHIFT_OFF + 8192u + ((m) - 32u) * 128u)

// v (x) K from K's 32 LDS columns at `base` (8 ds_read_b128 + 32 v_bitop3).
// (The generic gf2_mulmod here had its factor folded into 32 hoisted shifted
// copies: ~70 spilled VGPRs.)
__device__ __forceinline__ uint32_t stream_mulcol(uint32_t v, uint32_t base) {
  uint32_t p = 0;
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const u32x4 c = lds_ld128(base + g * 16u);
    p = __builtin_amdgcn_bitop3_b32(p, c.x, (uint32_t)((int32_t)(v << (4 * g + 0)) >> 31), 0x78);
    p = __builtin_amdgcn_bitop3_b32(p, c.y, (uint32_t)((int32_t)(v << (4 * g + 1)) >> 31), 0x78);
    p = __builtin_amdgcn_bitop3_b32(p, c.z, (uint32_t)((int32_t)(v << (4 * g + 2)) >> 31), 0x78);
    p = __builtin_amdgcn_bitop3_b32(p, c.w, (uint32_t)((int32_t)(v << (4 * g + 3)) >> 31), 0x78);
  }
  return p;
}

// The Horner shift v (x) x^(8*128*d), d = 0..63 (round 6): nibble tables
// instead of walk_mulcol's 32 bit columns (32 v_bfe_i32 + 32 v_bitop3 +
// 8 ds_read_b128).  d = 16h + f: v (x) K^f, then (x) K^(16h); each stage is
// 8 lookups of (nibble q at position j) (x) K^e, by linearity.  A lookup's
// address is one v_and_or_b32 of v shifted so that the nibble sits in the
// table's index bits.  The layout is chosen for the LDS banks (bank = address
// bits 2-6 within each 32-lane half of a ds_read_b32, MI355X_MICROARCH.md
// "LDS"): stage A (16 factors f) has f in bits 2-5 and q in bits 6-9, so
// two lanes of a half meet on a bank only when they share f and q's low
// bit; stage B (4 factors h) has q in bits 2-5 and h in bits 6-7, so lanes
// that share h -- a Horner's lanes mostly do -- never conflict (equal q is
// one address, a broadcast).  Modelled (tools/lds_conflicts.py) and counted
// (SQ_LDS_BANK_CONFLICT): 64 -> 16 extra LDS cycles per Horner of a tile
// without events, 128 -> 30 in an event tile, against round 6's first
// layout ([j][q][b] / [G][q][j'][a], whose stage-2 bank ignored q).
// 10 KiB over the walk columns' area (COLS + KHI, which this kernel does not
// otherwise use).
#define LDS_NIBA_OFF LDS_COLS_OFF            // [8 j][16 q][16 f] u32, 8 KiB
#define LDS_NIBB_OFF (LDS_COLS_OFF + 8192u)  // [8 j][4 h][16 q] u32, 2 KiB
static_assert((LDS_NIBA_OFF & 0x3FCu) == 0u && (LDS_NIBB_OFF & 0xFCu) == 0u, "the or-addressing needs these bits clear");
static_assert(LDS_NIBB_OFF + 2048u <= LDS_KLO_OFF, "the nibble tables end where the klo table starts");

// Tables of both stages: entry (j, q, e) = (q << 4j) (x) factor(e), with the
// stage-A factors e = f = 0..15 and the stage-B factors e = 16h (h = 0..3).
template <uint32_t NA, uint32_t NB, class F>
__device__ __forceinline__ void build_nib(F factor) {
  for (uint32_t i = threadIdx.x; i < 2560u; i += blockDim.x) {
    uint32_t addr, q, j, e;
    if (i < 2048u) {  // stage A: i = (j * 16 + q) * 16 + f
      const uint32_t f = i & 15u;
      q = (i >> 4) & 15u;
      j = i >> 8;
      e = f;
      addr = NA + 1024u * j + 64u * q + 4u * f;
    } else {  // stage B: k = (j * 4 + h) * 16 + q
      const uint32_t k = i - 2048u;
      q = k & 15u;
      const uint32_t h = (k >> 4) & 3u;
      j = k >> 6;
      e = 16u * h;
      addr = NB + 256u * j + 64u * h + 4u * q;
    }
    *(__attribute__((address_space(3))) uint32_t*)(size_t)addr = gf2_mulmod(q << (4u * j), factor(e));
  }
}

// v (x) factor(d), d = 0..63, from the tables build_nib<NA, NB> made
template <uint32_t NA, uint32_t NB>
__device__ __forceinline__ uint32_t nib_mul(uint32_t v, uint32_t d) {
  const uint32_t bA = NA + ((d & 15u) << 2), bB = NB + ((d >> 4) << 6);
  // stage A: nibble j of v at bits 6-9 of v shifted right by 4j - 6
  uint32_t u = __builtin_amdgcn_bitop3_b32(lds_ld(nullptr, ((v << 6) & 0x3C0u) | bA),
                                           lds_ld(nullptr, (((v << 2) & 0x3C0u) | bA) + 1024u),
                                           lds_ld(nullptr, (((v >> 2) & 0x3C0u) | bA) + 2048u), 0x96);
  u = __builtin_amdgcn_bitop3_b32(u, lds_ld(nullptr, (((v >> 6) & 0x3C0u) | bA) + 3072u),
                                  lds_ld(nullptr, (((v >> 10) & 0x3C0u) | bA) + 4096u), 0x96);
  u = __builtin_amdgcn_bitop3_b32(u, lds_ld(nullptr, (((v >> 14) & 0x3C0u) | bA) + 5120u),
                                  lds_ld(nullptr, (((v >> 18) & 0x3C0u) | bA) + 6144u), 0x96);
  u ^= lds_ld(nullptr, (((v >> 22) & 0x3C0u) | bA) + 7168u);
  // stage B: nibble j of u at bits 2-5 of u shifted right by 4j - 2
  uint32_t y = __builtin_amdgcn_bitop3_b32(lds_ld(nullptr, ((u << 2) & 0x3Cu) | bB),
                                           lds_ld(nullptr, (((u >> 2) & 0x3Cu) | bB) + 256u),
                                           lds_ld(nullptr, (((u >> 6) & 0x3Cu) | bB) + 512u), 0x96);
  y = __builtin_amdgcn_bitop3_b32(y, lds_ld(nullptr, (((u >> 10) & 0x3Cu) | bB) + 768u),
                                  lds_ld(nullptr, (((u >> 14) & 0x3Cu) | bB) + 1024u), 0x96);
  y = __builtin_amdgcn_bitop3_b32(y, lds_ld(nullptr, (((u >> 18) & 0x3Cu) | bB) + 1280u),
                                  lds_ld(nullptr, (((u >> 22) & 0x3Cu) | bB) + 1536u), 0x96);
  return y ^ lds_ld(nullptr, (((u >> 26) & 0x3Cu) | bB) + 1792u);
}

// The exact capture at an end at byte t of word u: the register s before the
// word advanced over the word's t bytes before the end (the ending record's
// last bytes), slicing-by-t from cx = s ^ u:
// (s >> 8t) ^ XOR_{i<t} T_{t-1-i}[cx byte i].  Run once per chunk after the
// chains, off their dependency path.
__device__ __forceinline__ uint32_t stream_capture(const unsigned char* smem, uint32_t cx, uint32_t u, uint32_t t,
                                                   uint32_t lo) {
  const uint32_t b0 = t == 1u ? lo : (t == 2u ? lo + 128u : (lo | 0x10000u));  // T_{t-1}
  const uint32_t b1 = t == 2u ? lo : lo + 128u;                                // T_{t-2}
  const uint32_t l0 = lds_ld(smem, __builtin_amdgcn_perm(cx, b0, 0x0c020400u));  // byte 0
  const uint32_t l1 = lds_ld(smem, __builtin_amdgcn_perm(cx, b1, 0x0c020500u));  // byte 1
  const uint32_t l2 = lds_ld(smem, __builtin_amdgcn_perm(cx, lo, 0x0c020600u));  // byte 2 (T0)
  return ((cx ^ u) >> (t << 3)) ^ (t >= 1u ? l0 : 0u) ^ (t >= 2u ? l1 : 0u) ^ (t >= 3u ? l2 : 0u);
}


// A caller's device batch takes the stream kernel when its records are sorted
// and do not overlap, at most STREAM_MAX_GAP bytes apart, record 0 is not
// empty and every later empty record sits at its predecessor's end.  Then every
// 4 KiB page a 128-byte chunk of [off[0], end) lies on holds a byte of some
// record, so the chunk loads touch only the caller's pages.
// A caller's batch: the eligibility check, four records per thread (off[]
// as two 16-byte loads and len[] as one when both arrays are 16-byte aligned,
// element loads otherwise); the next thread's first record comes from the
// next lane (lane 63 loads it).  The slices' cuts follow by binary search
// (stream_cuts, sorted by then).  One record per thread ran 0.18 ms on config
// 3; a fused check + cuts pass 0.31 ms.
// cut w, w = 0..S: the first record starting at or after off[0] + span *
// fraction(w) of the slice plan (lsmck_splan.h; cut S = n: every record
// belongs to exactly one slice).  Binary search.  (Interior cuts rounded to
// multiples of 64 records, for whole 256-byte output blocks, ran 0.03-0.07 ms
// slower on config 3: the byte balance of the small slices suffers.  Not kept.)
__device__ __forceinline__ void stream_cut(const CrcParams& P, uint32_t w, uint32_t S, uint32_t W) {
  const uint64_t n = P.nrec;
  if (w == S) {
    P.scuts[w] = n;
    return;
  }
  const uint64_t o0 = P.off[0], dend = P.off[n - 1] + P.len[n - 1];
  const uint64_t target = o0 + (uint64_t)((double)(dend - o0) * splan::fraction(w, S, W));
  uint64_t a = 0, b = n;
  while (a < b) {
    const uint64_t m = (a + b) >> 1;
    if (P.off[m] < target) a = m + 1; else b = m;
  }
  P.scuts[w] = a;
}

// The check also computes the cuts, in its first W + 1 threads: their binary
// searches (dependent loads) run inside the check's own bandwidth-bound pass
// instead of a launch of their own behind it (the cuts of an ineligible batch
// are never read: the stream kernel exits on the flag).
template <bool VEC>
__global__ __launch_bounds__(256) void stream_check(CrcParams P, uint32_t S, uint32_t W) {
  const uint64_t n = P.nrec;
  const uint32_t gt = blockIdx.x * 256u + threadIdx.x;
  if (gt == 0u) P.sflag[1] = 0u;  // the stream kernel's slice tickets
  if (gt <= S) stream_cut(P, gt, S, W);
  const uint64_t i0 = (uint64_t)gt * 4u;  // (threads past the records load record n-1 and find nothing)
  uint64_t o[5];
  uint32_t l[5];
  if (VEC && i0 + 4u <= n) {
    const u32x4 a = *(const u32x4*)(P.off + i0), b = *(const u32x4*)(P.off + i0 + 2u);
    const u32x4 c = *(const u32x4*)(P.len + i0);
    o[0] = ((uint64_t)a.y << 32) | a.x;
    o[1] = ((uint64_t)a.w << 32) | a.z;
    o[2] = ((uint64_t)b.y << 32) | b.x;
    o[3] = ((uint64_t)b.w << 32) | b.z;
    l[0] = c.x; l[1] = c.y; l[2] = c.z; l[3] = c.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint64_t i = i0 + j < n ? i0 + j : n - 1u;
      o[j] = P.off[i];
      l[j] = P.len[i];
    }
  }
  // the next thread's first record
  o[4] = ((uint64_t)(uint32_t)__shfl_down((int)(uint32_t)(o[0] >> 32), 1) << 32) | (uint32_t)__shfl_down((int)(uint32_t)o[0], 1);
  l[4] = (uint32_t)__shfl_down((int)l[0], 1);
  if ((threadIdx.x & 63u) == 63u && i0 + 4u < n) {
    o[4] = P.off[i0 + 4u];
    l[4] = P.len[i0 + 4u];
  }
  bool bad = i0 == 0 && n > 0 && l[0] == 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint64_t e = o[j] + l[j];
    bad = bad || (i0 + j + 1u < n && (o[j + 1] < e || o[j + 1] - e > STREAM_MAX_GAP || (l[j + 1] == 0u && o[j + 1] != e)));
  }
  if (bad) *P.sflag = 0u;  // plain stores of one value: no atomic needed
}

// the cuts alone (trusted batches: no check)
__global__ __launch_bounds__(256) void stream_cuts(CrcParams P, uint32_t S, uint32_t W) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w == 0u) P.sflag[1] = 0u;  // the stream kernel's slice tickets
  if (w > S || !*P.sflag) return;
  stream_cut(P, w, S, W);
}

// the tile's 64 chunks: bytes [tb, tb + 8192) from P.base (tb >= -127, the
// chunk grid is 128-byte aligned in memory); the buffer range ends in the
// dword holding the slice's last byte (end4), so loads past it read zeros and
// touch nothing: the tile at a cut is not read again by the slice before
// (c0, a slice's first tile: the chunks in front of the first record's chunk
// c0 belong to the slice before and are not fetched -- their lanes take an
// offset past the range and read zeros, which reach no result: the window
// holds no record of theirs and the first start resets its chain)
template <int ABLATE>
__device__ __forceinline__ void stream_issue(const CrcParams& P, int64_t tb, uintptr_t end4, uint32_t lane,
                                             uint32_t (&u)[32], uint32_t c0 = 0u) {
  const uintptr_t t0 = (uintptr_t)P.base + (uintptr_t)tb;
  const uint64_t span = end4 - t0;
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(P.base + tb), (short)0, (int)(span < 0x7FFFFFFFull ? span : 0x7FFFFFFFull), 0x00020000);
  const uint32_t vo = lane >= c0 ? lane * 128u : 0x80000000u;
  if (ABLATE == 2 || ABLATE == 4 || ABLATE == 10 || ABLATE == 11) {  // diagnostic: compute only (no payload loads; results invalid)
#pragma unroll
    for (int j = 0; j < 32; ++j) u[j] = (uint32_t)tb * 0x9E3779B1u + lane + j;
    return;
  }
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    auto v = __builtin_amdgcn_raw_buffer_load_b128(r, vo + 16u * g, 0, 0);
    u[4 * g + 0] = v[0];
    u[4 * g + 1] = v[1];
    u[4 * g + 2] = v[2];
    u[4 * g + 3] = v[3];
  }
  keep_live(vo);
}

// CRC of a short record (L < 64 bytes) ending at tile byte re (tile base tb):
// the 64-byte window [re-64, re) front-padded with zeros.  Only the dwords
// that intersect the record are loaded (the others read as zeros through an
// out-of-range buffer offset), so no byte outside the record's dwords is
// touched.  jmin (uniform): the first word any short lane of the wave needs.
__device__ __forceinline__ uint32_t stream_short(const CrcParams& P, const unsigned char* smem, int64_t tb, int32_t re,
                                                 uint32_t L, bool on, uint32_t jmin, uint32_t lo, uint32_t hi) {
  // buffer base 256 bytes in front of the tile (a short record ending in the
  // tile starts at tile byte -63 or later); only the record's dwords are
  // addressed, the others take an offset past the range
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(P.base + (tb - 256)), (short)0, 8192 + 256, 0x00020000);
  const uint32_t e = (uint32_t)(re + 256);  // the record's end in buffer offsets
  const uint32_t s = e - L;
  const uint32_t w0 = e - 64u;              // the window's first byte
  const uint32_t sh = (uint32_t)(((uintptr_t)P.base + (uintptr_t)(tb - 256) + w0) & 3u);
  const uint32_t p4 = w0 - sh;
  uint32_t d[17];
#pragma unroll
  for (int i = 0; i < 17; ++i) {
    const uint32_t a = p4 + 4u * i;
    const bool hit = on && a + 4u > s && a < e;  // the dword holds a record byte
    d[i] = __builtin_amdgcn_raw_buffer_load_b32(r, hit ? a : 0x80000000u, 0, 0);
  }
  const uint32_t lead = 64u - L;  // window bytes in front of the record (zeroed)
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if ((uint32_t)j < jmin) continue;  // (uniform) words no short lane of the wave needs
    uint32_t w = __builtin_amdgcn_alignbyte(d[j + 1], d[j], sh);
    const uint32_t b = 4u * j;
    w = (b + 4u <= lead) ? 0u : (b >= lead ? w : w & (0xFFFFFFFFu << ((lead - b) << 3)));
    c = crc_word(smem, c, w, lo, hi);
  }
  return ~(c ^ lds_ld(smem, LDS_TINIT_OFF + (L << 2)));
}

// the Horner shift of a chunk's value to its target chunk, d chunks on
__device__ __forceinline__ uint32_t horner(uint32_t v, uint32_t d) {
#ifdef LSMCK_HORNER_COLS
  return walk_mulcol(v, d);
#else
  return nib_mul<LDS_NIBA_OFF, LDS_NIBB_OFF>(v, d);
#endif
}

// the finish's factor: v (x) x^(8m), m = 0..63, from the bit columns.  (The
// nibble tables here too -- in the bank-aware layout as well: 18.94 against
// 18.58 ms, config 3w 19.8 against 19.3, profiles/r06/finish -- over the
// shift-by-32/96 and klo areas, ran slower:
// config 3 19.87-19.93 against 19.11-19.20 ms, config 3w 21.10-21.22 against
// 20.36-20.40 ms, same box, 4 / 3 interleaved rounds, profiles/r06/horner --
// the finish runs in the few lanes that hold a record, whose LDS reads cost
// per active lane, and its tables put the kernel at 8 spilled SGPRs.)
__device__ __forceinline__ uint32_t finish_mul(uint32_t v, uint32_t m) { return stream_mulcol(v, LDS_XMC_OFF(m)); }

#ifdef LSMCK_WAVE_DIAG
// Diagnostic builds only (EXTRA=-DLSMCK_WAVE_DIAG tools/build_ab.sh <name> WT;
// tools/wave_tail.py reads the dump): per wave, the constant 100 MHz clock at
// the kernel's entry and exit, its tile counts (event tiles << 32 | tiles
// without events) and where it ran (HW_ID | XCC_ID << 32).
#define LSMCK_WAVE_DIAG_MAX 8192u
__device__ uint64_t g_wave_diag[LSMCK_WAVE_DIAG_MAX][4];
#define WAVE_DIAG(...) __VA_ARGS__
#else
#define WAVE_DIAG(...)
#endif

template <int ABLATE = 0>
__global__ __launch_bounds__(1024) void crc32_stream_kernel(CrcParams P) {
  if (!*P.sflag) return;  // a caller's batch that is not sorted / packed enough: the walking kernel takes it
  WAVE_DIAG(const uint64_t diag_t0 = wall_clock64(); uint32_t diag_ev = 0; uint32_t diag_no = 0;)
  WAVE_DIAG(auto diag_out = [&] {
    const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if ((threadIdx.x & 63u) == 0u && w < LSMCK_WAVE_DIAG_MAX) {
      g_wave_diag[w][0] = diag_t0;
      g_wave_diag[w][1] = wall_clock64();
      g_wave_diag[w][2] = ((uint64_t)diag_ev << 32) | diag_no;
      g_wave_diag[w][3] = (uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
                          ((uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
    }
  };)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  build_lds_tables(smem, P);
  __syncthreads();  // the Horner tables reuse the cols + khi areas, the finish's x^(8m) the shift-by-32/96 tables' areas
#ifdef LSMCK_HORNER_COLS
  build_walk_cols(P);  // (A/B: round 5's bit-column Horner)
#else
  build_nib<LDS_NIBA_OFF, LDS_NIBB_OFF>([&](uint32_t e) { return P.kseg[e]; });  // x^(8*128*e)
#endif
  if (threadIdx.x >= 128u && threadIdx.x < 192u) {  // the finish factors' bit columns, x^(8m)
    const uint32_t f = threadIdx.x - 128u;
    uint32_t K = 0x80000000u;  // m zero-byte steps of the register from x^0
    for (uint32_t i = 0; i < f; ++i) K = (K >> 8) ^ lds_ld(smem, 256u * (K & 0xFFu));  // T0 (replica 0)
    const uint32_t base = LDS_XMC_OFF(f);
    for (uint32_t i = 0; i < 32u; ++i) {
      *(__attribute__((address_space(3))) uint32_t*)(size_t)(base + 4u * i) = K;
      K = (K >> 1) ^ (0xEDB88320u & (0u - (K & 1u)));
    }
  }
  const uint32_t lane = threadIdx.x & 63u;
  // this wave's event map: 64 chunks x {end in chain 0, start in chain 0, end
  // in chain 1, start in chain 1}, each the chain byte + 1 (0 = none)
  const uint32_t smap = LDS_SMAP_OFF + (threadIdx.x >> 6) * 256u;
  *(__attribute__((address_space(3))) uint32_t*)(size_t)(smap + 4u * lane) = 0u;
  __syncthreads();
  const uint32_t lo = (lane & 31u) * 4u, hi = lo | 0x10000u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const uint64_t n = P.nrec;
  // chunk grid origin, relative to P.base (128-byte aligned in memory)
  const int64_t a0 = (int64_t)((((uintptr_t)P.base + P.off[0]) & ~(uintptr_t)127) - (uintptr_t)P.base);
  // The batch is cut into P.nslice slices (stream_cut, by the plan of
  // lsmck_splan.h: a large first slice per wave, then groups of shrinking
  // ones), several per wave on a large batch.  A wave takes slice `wave`
  // first and then the next slice nobody has taken (a ticket counter behind the flag), until none
  // is left: the waves of a CU finish a launch up to 3 ms apart when each owns
  // one fixed share (tools/wave_tail.py), with the same tile counts -- the
  // SIMD's issue arbitration, not the work, decides -- and a wave that is done
  // early now goes on with work the late ones would have been left with.
  // (what a slice's start and end need of the launch is read from the kernel
  // arguments again, through a pointer the compiler cannot see through: held
  // in SGPRs across the tiles, these values were spilled)
  typedef __attribute__((address_space(4))) const CrcParams kargs_t;
  kargs_t* ka = (kargs_t*)__builtin_amdgcn_kernarg_segment_ptr();
  for (uint32_t slice = wave;;) {
  asm volatile("" : "+s"(ka));
  const uint32_t nslice = ka->nslice, nwaves = ka->nwaves;
  if (slice >= nslice) break;
  // The slice's records, where its first starts and where its last ends:
  // wave-uniform by construction, and said so explicitly -- a load through a
  // pointer that was itself loaded counts as divergent, and a buffer resource
  // built from such a value is formed in a per-lane loop around every load
  // (the slice's end held that way in the payload's range: 26.4-26.7 ms
  // against 17.1, profiles/r08/handover/ab_c3_parts.log).
  auto uni64 = [](uint64_t v) -> uint64_t {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  };
  const uint64_t r_lo = uni64(ka->scuts[slice]), r_hi = uni64(ka->scuts[slice + 1]);
  if (nslice > nwaves) {  // the next slice's ticket (a batch of one slice per wave takes none)
    uint32_t tk = 0;
    if (lane == 0u) tk = atomicAdd(ka->sflag + 1, 1u);
    slice = nwaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)tk);
  } else {
    slice = nslice;
  }
  if (r_lo >= r_hi) continue;  // no record in this slice
  const uint64_t o_lo = uni64(P.off[r_lo]), e_hi = uni64(P.off[r_hi - 1] + P.len[r_hi - 1]);
  const uint64_t t_first = (uint64_t)((int64_t)o_lo - a0) >> 13;
  const uint64_t t_last = (uint64_t)((int64_t)e_hi - a0) >> 13;
  const uint32_t c_first = (uint32_t)((uint64_t)((int64_t)o_lo - a0) >> 7) & 63u;  // the first record's chunk in its tile
  // the payload's range ends in the dword holding the slice's last byte
  const uintptr_t end4 = ((uintptr_t)P.base + e_hi + 3u) & ~(uintptr_t)3;
  // (a batch that is not sorted never gets here; the clamp keeps the loop
  // bounded whatever the descriptors hold)
  const uint64_t ntile = t_last >= t_first ? t_last - t_first + 1u : 0u;
  auto tbase = [&](uint64_t t) -> int64_t { return a0 + (int64_t)(t << 13); };

  // the window: off / len of records bt + lane (clamped to n - 1; masked at use)
  uint64_t Wo;
  uint32_t Wl;
  auto win_load = [&](uint64_t b) {
    const uint64_t i = b + lane;
    const uint64_t ic = i < n ? i : n - 1u;
    Wo = P.off[ic];
    Wl = P.len[ic];
  };
  uint64_t bt = r_lo;  // the first record that has not ended yet
  uint32_t carry = 0;  // the record open at the tile's end, its raw value aligned to the tile's end
  win_load(bt);
  // The CRCs are queued in one VGPR (lane p: record qb + p, qb a multiple of
  // 64) and stored as whole 256-byte blocks: a slice's records are
  // consecutive, so only its first and last blocks are partial.  Per-tile
  // stores of the ~5 records a tile ends wrote partial 128-byte lines (the
  // config-3 PMC counted 5.9 GB of fetches for the 0.27 GB output,
  // profiles/r02/official_b).
  uint32_t qv = 0;
  uint64_t qb = r_lo & ~63ull;
  uint32_t qs = (uint32_t)(r_lo & 63u), qf = qs;  // first valid lane of the block, next lane to fill
  auto qstore = [&](uint32_t v, bool on, uint32_t* out) {  // block qb from a uniform base: no 64-bit lane address to keep
    const __amdgpu_buffer_rsrc_t r =
        __builtin_amdgcn_make_buffer_rsrc((void*)(out + qb), (short)0, 256, 0x00020000);
    // (ABLATE 6, diagnostic: no output stores -- unless a magic value keeps the checksums alive)
    if (on && (ABLATE != 6 || v == 0x9E3779B1u)) __builtin_amdgcn_raw_buffer_store_b32(v, r, lane << 2, 0, 0);
  };
  auto qpush = [&](uint32_t v, uint32_t cnt) {  // window lanes 0 .. cnt-1: the next cnt records (cnt <= 64)
    const uint32_t src = (lane - qf) & 63u;
    const uint32_t val = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)v);
    const uint32_t end = qf + cnt;  // at most one block completes
    qv = (lane >= qf && lane < end) ? val : qv;
    if (end >= 64u) {
      qstore(qv, lane >= qs, P.out);
      qb += 64u;
      qs = 0u;
      qf = end - 64u;
      qv = lane < qf ? val : qv;
    } else {
      qf = end;
    }
  };

  // a tile without events: the straight chains, the Horner shift of every
  // chunk to the tile end and the carry.  The carry (the open record's raw
  // CRC up to this tile, aligned to its start) enters as lane 0's initial
  // register: the Horner shift of lane 0 then carries it to the tile end with
  // the chunk.
  auto bulk = [&](const uint32_t (&U)[32]) {
    if constexpr (ABLATE == 11 || ABLATE == 12) {  // diagnostic: four chains of 8 words, XOR for the combine (results invalid)
      uint32_t y0 = U[0] ^ (lane == 0u ? carry : 0u), y1 = U[8], y2 = U[16], y3 = U[24];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        y0 = crc_step_x(smem, y0, k + 1 < 8 ? U[k + 1] : 0u, lo, hi);
        y1 = crc_step_x(smem, y1, k + 1 < 8 ? U[9 + k] : 0u, lo, hi);
        y2 = crc_step_x(smem, y2, k + 1 < 8 ? U[17 + k] : 0u, lo, hi);
        y3 = crc_step_x(smem, y3, k + 1 < 8 ? U[25 + k] : 0u, lo, hi);
      }
      uint32_t dy = 63u - lane;
      asm volatile("" : "+v"(dy));
      const uint32_t XY = wave_prefix_xor(horner(shift_bytes32<2>(smem, y0 ^ y1) ^ y2 ^ y3, dy));
      carry = (uint32_t)__builtin_amdgcn_readlane((int)XY, 63);
      return;
    }
    uint32_t z0 = U[0] ^ (lane == 0u ? carry : 0u), z1 = U[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      z0 = crc_step_x(smem, z0, k + 1 < 16 ? U[k + 1] : 0u, lo, hi);
      z1 = crc_step_x(smem, z1, k + 1 < 16 ? U[17 + k] : 0u, lo, hi);
    }
    uint32_t dz = 63u - lane;
    asm volatile("" : "+v"(dz));  // not hoisted: eight loop-invariant column addresses spilled
    const uint32_t XZ = wave_prefix_xor(horner(shift_bytes32<2>(smem, z0) ^ z1, dz));
    carry = (uint32_t)__builtin_amdgcn_readlane((int)XZ, 63);
  };

  auto process = [&](const uint32_t (&U)[32], uint64_t t, auto&& issue_next) {
    const int64_t tb = tbase(t);
    if constexpr (ABLATE == 9 || ABLATE == 10 || ABLATE == 11) {  // diagnostic: the bulk chains + Horner alone, no window / map
      issue_next();                               // (10: without the payload loads); results invalid
      __builtin_amdgcn_sched_barrier(0);
      bulk(U);
      return;
    }
    // No event in the tile, decided from record bt alone (scalar): it ends
    // past the tile (then so does every later record) and it did not start
    // here as a long record.  Such a tile skips the map and the window slide.
    bool zf = false;
    if constexpr (ABLATE == 0 || ABLATE >= 6) {
      const uint32_t so_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)Wo);
      const uint32_t so_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(Wo >> 32));
      const uint32_t sl = (uint32_t)__builtin_amdgcn_readfirstlane((int)Wl);
      const int64_t s0 = (int64_t)(((uint64_t)so_hi << 32) | so_lo) - tb;
      zf = bt >= r_hi || (s0 + (int64_t)sl >= 8192 && (s0 < 0 || sl < STREAM_LONG));
    }
    // --- map: the window's records that end in this tile write their events
    // (long records) into the wave's LDS map; a tile in which all 64 window
    // records end walks the next window too (rare: records of ~128 B or less)
    uint32_t Kw = 0;       // (uniform) words holding an event: chain 0 bits 0-15, chain 1 bits 16-31
    bool shorts = false;   // (uniform) a short record ends in this tile
    uint64_t wb = bt;      // base of the window being mapped
    uint32_t nwin = 0;     // full windows (64 records ending here) before the last one
    uint32_t cntw = 0;     // records of the last window ending here
    int32_t re = 8191, rs = 8191;  // the last window's tile-relative end and start (start clamped to >= -128)
    bool lng = false, sin = false;  // long record; its start lies in this tile
    const uint64_t bt0 = bt;
    bool z = zf;
    if (!zf) {
      for (;;) {
        const int64_t e64 = (int64_t)(Wo + Wl) - tb, s64 = (int64_t)Wo - tb;
        const bool inr = wb + lane < r_hi;
        const bool ends = inr && e64 < 8192;
        cntw = (uint32_t)__builtin_popcountll(__ballot(ends));
        lng = Wl >= STREAM_LONG;
        sin = inr && s64 >= 0 && s64 < 8192;
        re = (int32_t)(ends ? e64 : 8191);
        rs = (int32_t)(s64 < -128 ? -128 : (s64 > 8191 ? 8191 : s64));
        const bool ev_e = ends && lng, ev_s = sin && lng;
        typedef __attribute__((address_space(3))) unsigned char lds_u8w_t;
        if (ev_e) *(lds_u8w_t*)(size_t)(smap + 4u * ((uint32_t)re >> 7) + (((uint32_t)re >> 5) & 2u)) = (unsigned char)((re & 63) + 1);
        if (ev_s) *(lds_u8w_t*)(size_t)(smap + 4u * ((uint32_t)rs >> 7) + (((uint32_t)rs >> 5) & 2u) + 1u) = (unsigned char)((rs & 63) + 1);
        Kw |= wave_or_u32((ev_e ? 1u << (((uint32_t)re & 127u) >> 2) : 0u) | (ev_s ? 1u << (((uint32_t)rs & 127u) >> 2) : 0u));
        shorts = shorts || __any(ends && !lng);
        if (cntw < 64u) break;
        wb += 64u;
        ++nwin;
        win_load(wb);  // (a dependent load: tiles of many small records only)
      }
      bt = wb + cntw;
      // no event at all: no record ends here, and the open record started before
      z = nwin == 0u && cntw == 0u && !__builtin_amdgcn_readfirstlane((int)(sin && lng));
      // the next tile's window: this one shifted by cntw (lands while this tile is checksummed)
      const uint32_t src = lane + cntw;
      const int sp = (int)((src & 63u) << 2);
      const uint32_t wlo = (uint32_t)__builtin_amdgcn_ds_bpermute(sp, (int)(uint32_t)Wo);
      const uint32_t whi = (uint32_t)__builtin_amdgcn_ds_bpermute(sp, (int)(uint32_t)(Wo >> 32));
      const uint32_t wl = (uint32_t)__builtin_amdgcn_ds_bpermute(sp, (int)Wl);
      Wo = ((uint64_t)whi << 32) | wlo;
      Wl = wl;
      if (src >= 64u) {  // the new entries only
        const uint64_t i2 = bt + lane;
        const uint64_t ic = i2 < n ? i2 : n - 1u;
        Wo = P.off[ic];
        Wl = P.len[ic];
      }
    }
    // then the payload one tile ahead: after the window, so that waiting for
    // the window at the next tile never waits for that payload; issued at the
    // top wave priority, so the eight loads enter the memory pipeline ahead of
    // the other waves' checksum work (config 3 19.64 -> 19.38 ms median over 8
    // same-box rounds, profiles/r03/x)
    __builtin_amdgcn_s_setprio(3);
    issue_next();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(0);
    if constexpr (ABLATE == 0 || ABLATE >= 4) {
      // (ABLATE 4 / 5, diagnostic: every tile takes this path -- the bulk
      // chains + Horner cost without / with the payload loads)
      if (z || ABLATE == 4 || ABLATE == 5 || ABLATE == 12) {  // (uniform) no event in the tile
        WAVE_DIAG(++diag_no;)
        bulk(U);
        return;
      }
    }
    // An event tile runs at wave priority 1 (above the bulk tiles' 0, below
    // the payload issue's 3): the VALU-heavy event bodies win the issue
    // arbitration over waves whose bulk chains wait on the LDS.  Same box,
    // 3 interleaved rounds: config 3 19.09-19.14 -> 18.87-18.88 ms, config 3w
    // 19.61-19.68 -> 19.21-19.32 (profiles/r06/prio; priority 2 over the word
    // loop alone 18.90 / 19.23).
    __builtin_amdgcn_s_setprio(1);
    WAVE_DIAG(++diag_ev;)
    // --- chunk-lane view: this chunk's events (byte + 1 in its chain, 0 = none)
    typedef __attribute__((address_space(3))) uint32_t lds_u32w_t;
    uint32_t ev = *(lds_u32w_t*)(size_t)(smap + 4u * lane);
    if (ev) *(lds_u32w_t*)(size_t)(smap + 4u * lane) = 0u;
    const uint64_t M1 = __ballot((ev & 0x00FF00FFu) != 0u);  // chunks holding an end
    const uint64_t Ms = __ballot((ev & 0xFF00FF00u) != 0u);  // chunks holding a start
    const bool ke0 = __any((ev & 0xFFu) != 0u), ke1 = __any((ev & 0xFF0000u) != 0u);
    if (ABLATE == 3) {  // diagnostic: payload loads only
      uint32_t x = 0;
#pragma unroll
      for (int k = 0; k < 32; ++k) x ^= U[k];
      if (x == 0x9E3779B1u) P.out[0] = x ^ ev;
      __builtin_amdgcn_s_setprio(0);
      return;
    }
    // --- the chunk's two chains: resets at the starts, captures at the ends.
    // A word's branch (uniform: some lane has an event there) only selects
    // the two steps' inputs; both steps follow it, so their eight lookups
    // issue together.  The carry enters as lane 0's initial register: up to
    // the tile's first start it rides in lane 0's chain, into that record's
    // capture, R0 or the Horner value of chunk 0; a reset drops it.
    uint32_t c0 = U[0] ^ (lane == 0u ? carry : 0u), c1 = U[16], x0 = 0u, x1 = 0u, ub0 = 0u, ub1 = 0u;
    // (ABLATE 8, diagnostic: no per-word event bodies -- results invalid)
    const uint32_t Km = ABLATE == 8 ? 0u : Kw;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t w0 = k + 1 < 16 ? U[k + 1] : 0u, w1 = k + 1 < 16 ? U[17 + k] : 0u;
      uint32_t i0 = c0, i1 = c1, n0 = w0, n1 = w1;
      // each chain's body only where some lane has an event in that chain's
      // word k (uniform), not wherever either chain has one
      // The body's assignments run under the EXEC mask, on the lanes that hold
      // the event (one or two of the 64), as plain moves: as selects on SGPR
      // masks (v_cndmask_b32_e64, half rate: tools/microbench_valu.hip) every
      // lane paid four of them per chain and word.  The empty asm on the
      // assigned values keeps the blocks from being if-converted back.
      // All four fields of ev are decoded by one add: b + 3 <= 67 carries into
      // no neighbour, and chain byte j = b - 1 lies in word k  <=>
      // (b + 3) >> 2 == k + 1 (b = 0, no event, gives 0); a packed boundary's
      // end and start (equal fields) share that decode.
      if (Km & (1u << k)) {
        uint32_t e = ev;
        asm volatile("" : "+v"(e));  // recomputed here, not hoisted: fewer VGPRs through the loop
        const uint32_t e3 = e + 0x03030303u;
        if (((e3 >> 2) & 0x3Fu) == (uint32_t)(k + 1)) {
          x0 = c0;
          ub0 = U[k];
          asm volatile("" : "+v"(x0), "+v"(ub0));
        }
        if (((e3 >> 10) & 0x3Fu) == (uint32_t)(k + 1)) {
          const uint32_t mlo0 = (1u << ((e3 >> 5) & 0x18u)) - 1u;  // the word's bytes in front of the start
          i0 = ~(U[k] | mlo0);
          n0 = w0 ^ mlo0;
          asm volatile("" : "+v"(i0), "+v"(n0));
        }
      }
      if (Km & (1u << (16 + k))) {
        uint32_t e = ev;
        asm volatile("" : "+v"(e));
        const uint32_t e3 = e + 0x03030303u;
        if (((e3 >> 18) & 0x3Fu) == (uint32_t)(k + 1)) {
          x1 = c1;
          ub1 = U[16 + k];
          asm volatile("" : "+v"(x1), "+v"(ub1));
        }
        if ((e3 >> 26) == (uint32_t)(k + 1)) {
          const uint32_t mlo1 = (1u << ((e3 >> 21) & 0x18u)) - 1u;
          i1 = ~(U[16 + k] | mlo1);
          n1 = w1 ^ mlo1;
          asm volatile("" : "+v"(i1), "+v"(n1));
        }
      }
      crc_step_x2(c0, c1, i0, n0, i1, n1, lo, hi);
    }
    const uint32_t cap0 = ke0 ? stream_capture(smem, x0, ub0, ((ev & 0xFFu) - 1u) & 3u, lo) : 0u;
    const uint32_t cap1 = ke1 ? stream_capture(smem, x1, ub1, (((ev >> 16) & 0xFFu) - 1u) & 3u, lo) : 0u;
    const uint32_t R0 = c0;
    const uint32_t T = (ev >> 24) ? c1 : (shift_bytes32<2>(smem, c0) ^ c1);
    // --- Horner inside the tile: T to the chunk before the next END's chunk
    uint32_t l1 = lane + 1u;
    asm volatile("" : "+v"(l1));  // not hoisted: the loop-invariant lane mask spilled (a vmcnt(0) reload)
    const uint64_t above = lane == 63u ? 0ull : (M1 >> l1) << l1;
    const uint32_t cn = above ? (uint32_t)__builtin_ctzll(above) : 64u;
    const uint32_t X = wave_prefix_xor(horner(T, cn - 1u - lane));
    // --- records: the window lane of a record finishes it
    auto finish = [&](uint32_t cnt, int32_t re_, int32_t rs_, bool lng_, bool sin_) -> uint32_t {
      const uint32_t c = (uint32_t)re_ >> 7, j = (uint32_t)re_ & 127u;
      const uint32_t Ye = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((c - 1u) & 63u) << 2), (int)X);
      const uint32_t cs = (uint32_t)rs_ >> 7;
      const uint32_t Ys = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((cs - 1u) & 63u) << 2), (int)X);
      const uint32_t H = (c ? Ye : 0u) ^ ((sin_ && cs) ? Ys : 0u);
      const int sc = (int)(c << 2);
      const uint32_t R0c = (uint32_t)__builtin_amdgcn_ds_bpermute(sc, (int)R0);
      const uint32_t A0c = (uint32_t)__builtin_amdgcn_ds_bpermute(sc, (int)cap0);
      const uint32_t A1c = (uint32_t)__builtin_amdgcn_ds_bpermute(sc, (int)cap1);
      const bool in = lane < cnt;
      uint32_t fv = 0u;
      // only the lanes holding a long record from here on (a few per tile):
      // the LDS reads below cost per active lane
      if (in && lng_ && ABLATE != 7) {  // (ABLATE 7, diagnostic: no finish multiply -- results invalid)
        const bool h = j >= 64u;
        const uint32_t Pv = h ? (shift_bytes32<2>(smem, H) ^ R0c) : H;
        fv = ~(finish_mul(Pv, j & 63u) ^ (h ? A1c : A0c));
      }
      return fv;
    };
    auto finish_short = [&](uint32_t fv, uint32_t cnt, int32_t re_, int32_t rs_, bool lng_) -> uint32_t {
      const bool sh = lane < cnt && !lng_;
      const uint32_t L = sh ? (uint32_t)(re_ - rs_) : 0u;
      // (uniform) the first word any short lane needs: 16 - max over lanes of ceil(L / 4)
      const int need = sh ? (int)((L + 3u) >> 2) : 0;
      const uint32_t jmin = 16u - (uint32_t)__builtin_amdgcn_readlane(wave_prefix_max(need), 63);
      const uint32_t v = stream_short(P, smem, tb, re_, L, sh, jmin, lo, hi);
      return sh ? v : fv;
    };
    for (uint32_t k = 0; k < nwin; ++k) {  // full windows before the last (rare): reloaded
      const uint64_t i = bt0 + 64u * k + lane;  // < r_hi: every record of a full window ends here
      const uint64_t o = P.off[i];
      const uint32_t l = P.len[i];
      const int64_t s64 = (int64_t)o - tb;
      const int32_t kre = (int32_t)((int64_t)(o + l) - tb);
      const int32_t krs = (int32_t)(s64 < -128 ? -128 : s64);
      const bool klng = l >= STREAM_LONG;
      uint32_t fv = finish(64u, kre, krs, klng, s64 >= 0);
      if (__any(!klng)) fv = finish_short(fv, 64u, kre, krs, klng);
      qpush(fv, 64u);
    }
    if (cntw) {
      uint32_t fv = finish(cntw, re, rs, lng, sin);
      if (shorts && __any(lane < cntw && !lng)) fv = finish_short(fv, cntw, re, rs, lng);
      // pushed at once (round 5: holding them to the next tile, after its
      // payload issue, ran 0.1 ms slower on config 3; profiles/r05/f)
      qpush(fv, cntw);
    }
    // --- carry: the record open at the tile's end started at the tile's last start
    const uint32_t X63 = (uint32_t)__builtin_amdgcn_readlane((int)X, 63);
    const uint32_t cl = Ms ? 63u - (uint32_t)__builtin_clzll(Ms) : 0u;
    carry = X63 ^ (cl ? (uint32_t)__builtin_amdgcn_readlane((int)X, (int)(cl - 1u)) : 0u);
    __builtin_amdgcn_s_setprio(0);
  };

  // payload slots: one tile in flight while one is checksummed; tiles past
  // the run reload its last tile (in bounds, unused)
  auto tcl = [&](uint64_t x) -> int64_t { return tbase(x < ntile ? t_first + x : t_last); };
  auto none = [] {};
  uint32_t U0[32], U1[32];
  uint64_t i = 0;
  stream_issue<ABLATE>(P, tcl(0), end4, lane, U0, c_first);
  for (; i + 2 <= ntile; i += 2) {
    process(U0, t_first + i, [&] { stream_issue<ABLATE>(P, tcl(i + 1), end4, lane, U1); });
    process(U1, t_first + i + 1, [&] { stream_issue<ABLATE>(P, tcl(i + 2), end4, lane, U0); });
  }
  if (i < ntile) process(U0, t_first + i, none);
  if ((ABLATE == 4 || ABLATE == 5 || ABLATE == 7 || ABLATE >= 9) && carry == 0x9E3779B1u) P.out[0] = carry;  // keeps the ablated chains (and loads) alive
  if (ABLATE == 3) continue;
  asm volatile("" : "+s"(ka));  // (as above: P.out, kept for this one store, was spilled)
  qstore(qv, lane >= qs && lane < qf, ka->out);
  }  // (the wave's next slice)
  WAVE_DIAG(diag_out();)
}
}  // namespace lsmck

// ---------------------------------------------------------------------------
// Launchers (C linkage inside the library; the public C ABI is lsmck_api.cpp)
using namespace lsmck;


template <bool FAST, bool PERCOL>
static int launch_fixed(const CrcParams* P, int ncu, hipStream_t st) {
  size_t lds = LDS_SCRATCH_OFF;
  hipError_t e = hipFuncSetAttribute((const void*)crc32_fixed_kernel<FAST, 2, 0, PERCOL>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return -(int)e;
  hipLaunchKernelGGL((crc32_fixed_kernel<FAST, 2, 0, PERCOL>), dim3(ncu), dim3(1024), lds, st, *P);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

template <int ABLATE>
static int launch_wring(const CrcParams* P, int ncu, hipStream_t st) {
  size_t lds = LDS_SCRATCH_OFF;
  hipError_t e = hipFuncSetAttribute((const void*)crc32_wring_kernel<2, ABLATE>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return -(int)e;
  hipLaunchKernelGGL((crc32_wring_kernel<2, ABLATE>), dim3(ncu), dim3(1024), lds, st, *P);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// fixed-stride records: the whole-tile ring kernel for dword-aligned records
// whose segment count divides 64 (every tile starts on a record) and whose
// tile spans fit a buffer window; the two-slot segment kernel otherwise.
// variant bits 8-11: crc_ablate (3: payload loads only, ring kernel)
extern "C" int lsmk_launch_crc32_fixed(const CrcParams* P, int ncu, int variant, hipStream_t st) {
  const bool fast = ((uintptr_t)P->base % 4 == 0) && (P->stride % 4 == 0) && (P->flen % 128 == 0);
  const uint32_t nsegr = segs_of(P->flen);
  const bool percol = (64u % nsegr) == 0;
  const bool buf_ok = (uint64_t)P->stride * 65u + P->flen < (1ull << 31);
  const int ablate = (variant >> 8) & 0xF;
  if (fast && percol && buf_ok) return ablate == 3 ? launch_wring<3>(P, ncu, st) : launch_wring<0>(P, ncu, st);
  if (fast && percol) return launch_fixed<true, true>(P, ncu, st);
  if (fast) return launch_fixed<true, false>(P, ncu, st);
  return launch_fixed<false, false>(P, ncu, st);
}

// Slices of a stream batch and where their cuts lie: lsmck_splan.h.  A slice
// costs its wave a restart -- the window, a first tile that is not
// prefetched, the tile at the cut read by both neighbours -- so the smallest
// is kept at tens of tiles.
extern "C" uint32_t lsmk_stream_slices_max(int ncu) { return splan::slices_max(ncu); }

// whether this library carries the stream kernel's diagnostic ablations (crc_ablate 2, 4..10)
extern "C" int lsmk_ab_ablations() {
#ifdef LSMCK_AB_ABLATIONS
  return 1;
#else
  return 0;
#endif
}

// stream kernel: eligibility flag (trusted: the library's own batch, sorted
// with its gaps inside one buffer, so no check), the slices' cuts, the kernel.
// The walking kernel launched after it on the same stream exits when the flag
// is set.
extern "C" int lsmk_launch_crc32_stream(const CrcParams* P, int ncu, int variant, int trusted, hipStream_t st) {
  const uint64_t n = P->nrec;
  if (n == 0) return 0;
  hipError_t e = hipMemsetAsync(P->sflag, 1, 4, st);
  if (e != hipSuccess) return -(int)e;
  const uint32_t W = splan::slices(ncu, n), NW = splan::waves(ncu);
  if (!trusted) {  // a caller's batch: checked first, the cuts computed inside the check
    const bool vec = ((uintptr_t)P->off % 16u == 0) && ((uintptr_t)P->len % 16u == 0);
    const uint64_t nb = std::max<uint64_t>((n + 1023) / 1024, (W + 1u + 255u) / 256u);
    const dim3 g((unsigned)nb);
    if (vec) hipLaunchKernelGGL(stream_check<true>, g, dim3(256), 0, st, *P, W, NW);
    else hipLaunchKernelGGL(stream_check<false>, g, dim3(256), 0, st, *P, W, NW);
  } else {
    hipLaunchKernelGGL(stream_cuts, dim3((W + 1u + 255u) / 256u), dim3(256), 0, st, *P, W, NW);
  }
  const int ablate = (variant >> 8) & 0xF;
#ifdef LSMCK_AB_ABLATIONS
  // the stream kernel's diagnostic ablations: only in the
  // A/B libraries tools/build_ab.sh builds with EXTRA=-DLSMCK_AB_ABLATIONS
  const void* fn = ablate == 11 ? (const void*)crc32_stream_kernel<11>
                 : ablate == 12 ? (const void*)crc32_stream_kernel<12>
                 : ablate == 9 ? (const void*)crc32_stream_kernel<9>
                 : ablate == 10 ? (const void*)crc32_stream_kernel<10>
                 : ablate == 4 ? (const void*)crc32_stream_kernel<4>
                 : ablate == 5 ? (const void*)crc32_stream_kernel<5>
                 : ablate == 6 ? (const void*)crc32_stream_kernel<6>
                 : ablate == 7 ? (const void*)crc32_stream_kernel<7>
                 : ablate == 8 ? (const void*)crc32_stream_kernel<8>
                 : ablate == 3 ? (const void*)crc32_stream_kernel<3>
                 : ablate == 2 ? (const void*)crc32_stream_kernel<2> : (const void*)crc32_stream_kernel<0>;
#else
  // the product library: the kernel and its loads-only twin (the bench's
  // loads_only_ceiling); lsmck_ctx_set_option refuses the other ablations
  const void* fn = ablate == 3 ? (const void*)crc32_stream_kernel<3> : (const void*)crc32_stream_kernel<0>;
#endif
  const size_t lds = LDS_SCRATCH_OFF + LDS_SMAP_BYTES;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return -(int)e;
  CrcParams Q = *P;
  Q.nslice = W;
  Q.nwaves = NW;
  void* args[] = {(void*)&Q};
  e = hipLaunchKernel(fn, dim3(ncu), dim3(1024), args, lds, st);
  if (e != hipSuccess) return -(int)e;
  e = hipGetLastError();
#ifdef LSMCK_WAVE_DIAG
  // append this launch's marks to the file LSMCK_WAVE_DIAG_OUT names: a header
  // {magic, waves, records, 0} and four u64 per wave (waits for the launch)
  if (const char* path = getenv("LSMCK_WAVE_DIAG_OUT")) {
    const uint32_t nw = std::min<uint32_t>((uint32_t)ncu * 16u, LSMCK_WAVE_DIAG_MAX);
    std::vector<uint64_t> h(4u * (nw + 1u));
    h[0] = 0x4741494445564157ull;
    h[1] = nw;
    h[2] = n;
    h[3] = 0;
    if (hipStreamSynchronize(st) == hipSuccess &&
        hipMemcpyFromSymbol(h.data() + 4, HIP_SYMBOL(g_wave_diag), 32u * nw) == hipSuccess) {
      if (FILE* f = fopen(path, "ab")) {
        fwrite(h.data(), 8, h.size(), f);
        fclose(f);
      }
    }
  }
#endif
  return e == hipSuccess ? 0 : -(int)e;
}

extern "C" uint64_t lsmk_walk_sb_count(uint64_t n) { return (n + WALK_SB - 1) / WALK_SB; }

// walking descriptor kernel: superblock sums, their scan (total at
// P->total_segs), the kernel; sb_prefix holds lsmk_walk_sb_count(n) u64.
// Nothing is read back: asynchronous on st.
extern "C" int lsmk_launch_crc32_walk(const CrcParams* P, uint64_t* sb_prefix, int ncu, int variant,
                                      hipStream_t st) {
  const uint64_t n = P->nrec;
  if (n == 0) return 0;
  const uint64_t nsb = lsmk_walk_sb_count(n);
  const uint64_t nblk = std::min<uint64_t>((nsb + 15) / 16, (uint64_t)ncu * 2u);
  hipLaunchKernelGGL(walk_phase1, dim3((unsigned)nblk), dim3(1024), 0, st, P->len, n, sb_prefix,
                     (const uint32_t*)P->sflag);
  hipLaunchKernelGGL(scan_phase2, dim3(1), dim3(1024), 0, st, sb_prefix, (uint32_t)nsb, P->total_segs,
                     (const uint32_t*)P->sflag);
  CrcParams Q = *P;
  Q.sb_prefix = sb_prefix;
  const int ablate = (variant >> 8) & 0xF;
  const void* fn = ablate == 3 ? (const void*)crc32_walk_kernel<2, 3> : (const void*)crc32_walk_kernel<2>;
  size_t lds = LDS_SCRATCH_OFF;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return -(int)e;
  void* args[] = {(void*)&Q};
  e = hipLaunchKernel(fn, dim3(ncu), dim3(1024), args, lds, st);
  if (e != hipSuccess) return -(int)e;
  e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// ---------------------------------------------------------------------------
// Verify: n_bad += (crc[i] != expected[i]); first_bad = min i with a mismatch.
namespace lsmck {
__global__ __launch_bounds__(256) void crc32_compare_kernel(const uint32_t* __restrict__ crc,
                                                             const uint32_t* __restrict__ expected, uint64_t n,
                                                             unsigned long long* __restrict__ n_bad,
                                                             unsigned long long* __restrict__ first_bad) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long bad = 0, first = ~0ull;
  for (; i < n; i += stride) {
    if (crc[i] != expected[i]) {
      ++bad;
      if (i < first) first = i;
    }
  }
  if (bad) {
    atomicAdd(n_bad, bad);
    atomicMin(first_bad, first);
  }
}
}  // namespace lsmck

extern "C" int lsmk_launch_crc32_compare(const uint32_t* crc, const uint32_t* expected, uint64_t n,
                                          unsigned long long* n_bad, unsigned long long* first_bad, hipStream_t st) {
  if (n == 0) return 0;
  uint64_t blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(crc32_compare_kernel, dim3((unsigned)blocks), dim3(256), 0, st, crc, expected, n, n_bad,
                     first_bad);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
