// lsmck_device.h -- parameter blocks shared by the HIP kernels and the host
// dispatcher (lsmck_api.cpp).  Internal to liblsmck.so; not part of the C ABI.
#ifndef LSMCK_DEVICE_H
#define LSMCK_DEVICE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsmck.h"

namespace lsmck {

// CRC-32 batch job.  Records are either fixed ([r*stride, r*stride+flen)) or
// described by (off[r], len[r]) relative to `base`.
struct CrcParams {
  const unsigned char* base;
  const uint64_t* off;        // descriptor mode
  const uint32_t* len;        // descriptor mode
  uint64_t stride;            // fixed mode
  uint32_t flen;              // fixed mode
  uint64_t nrec;
  uint64_t* total_segs;       // walking kernel scratch: total segments (device)
  uint32_t* out;              // nrec CRCs
  const uint32_t* kseg;       // x^(8*128*k) mod P, k < 2^16
  const uint32_t* khi;        // x^(8*128*65536*k) mod P, k < 2^16
  const uint32_t* tinit;      // 0xFFFFFFFF (x) x^(8*m) mod P, m = 0..128; [129] = 0
  const uint32_t* master;     // slicing-by-4 tables T0..T3 (4 x 256), then shift tables ST_1..ST_3 (3 x 4 x 256)
  const uint32_t* zero;       // 256 zero bytes (16-aligned): the load window of empty segments
  const uint64_t* sb_prefix;  // walking descriptor kernel: exclusive segment prefix per WALK_SB-record superblock
  uint32_t* sflag;            // stream kernel: nonzero = it takes the batch (the walking kernel then exits)
  uint64_t* scuts;            // stream kernel: first record of each slice (slices + 1 entries)
  uint32_t nslice;            // stream kernel: slices of this launch (set by its launcher)
  uint32_t nwaves;            // stream kernel: waves of this launch (set by its launcher)
};

// SHA-256 batch job (lane per message).
struct ShaParams {
  const unsigned char* base;
  const uint64_t* off;        // null -> fixed mode
  const uint32_t* len;
  uint64_t stride;
  uint32_t flen;
  uint64_t nmsg;
  const uint32_t* order;      // optional permutation (longest first), may be null
  unsigned char* out;         // 32 bytes per message
  uint32_t pair;              // 1: two blocks per load window (A/B, lsmck_sha256.hip ShaWin2)
  const uint64_t* split;      // device: order index where the short tail starts (lean kernel), null = none
};

// One slice of a message streamed through sha256_slices_kernel.
#define SHA_SLICE_FIRST 1u
#define SHA_SLICE_LAST 2u
struct ShaSlice {
  uint64_t off;    // slice bytes at base + off
  uint64_t total;  // the message's length (used on its last slice)
  uint32_t len;    // slice bytes: a multiple of 64 unless it is the message's last slice
  uint32_t slot;   // state slot (8 u32) carrying the message between slices
  uint32_t msg;    // message index: digest at out + 32 * msg
  uint32_t flags;  // SHA_SLICE_FIRST | SHA_SLICE_LAST
};
struct ShaSliceParams {
  const unsigned char* base;
  const ShaSlice* slices;
  uint64_t nslices;
  uint32_t* state;
  unsigned char* out;
};

// The batch memtable build's workspace (lsmck_memtable.hip; carved out of one
// allocation by lsmk_mem_carve).  Per position of the order: perm (the
// command there), grp (its group's head position), head (its key differs from
// its predecessor's).  Per active slot of a round: apos (its position; apos2
// the next round's), chunk / tail / g / idx (the element's sort fields and
// command), o1..o3 (the slots' order after each sort pass), kout (the passes'
// sorted keys, unused), bnd / hd (run starts and their max-scan), act / ex
// (flags and their exclusive scan: the round's still-active slots; at the end
// the live positions and their output slots, n + 1 entries).
struct MemWs {
  uint64_t *chunk, *kout;
  uint32_t *perm, *grp, *apos, *apos2, *g, *idx, *o1, *o2, *o3, *bnd, *hd, *act, *ex;
  uint8_t *tail, *head;
};

// The batch write plan's arrays (lsmck_writeplan.hip; lsmk_wpl_carve lays them
// over a MemWs whose rounds are done).  perm / head: the build's order.  Per
// command: aw (klen + vlen and the Insert bit), prev (the command before with
// its key), mark (a memtable starts here), seg1 (its segment's number plus
// one).  Per candidate start: nxt / byt / state (its walk's outcome, and the
// chain's for a LONG start), exitp (the last start of its orbit inside its
// block).  Per position of the order: act / ex (it is an entry; its slot;
// n + 1).  Per entry: ekey / eval (segment and command in key order), skey /
// sval (by segment, then key).
struct WplWs {
  uint64_t *aw, *byt;
  uint32_t *perm, *prev, *nxt, *exitp, *mark, *seg1, *act, *ex, *ekey, *eval, *skey, *sval;
  uint8_t *head, *state;
};

// The batch command stream's own arrays (lsmck_apply.hip; lsmk_apl_carve lays
// them over what the write plan leaves free at the time).  ans: per command,
// the last write before it with its key -- what answers a Get -- in the one
// array of the workspace the plan never uses (apos2).  During prep, over the
// entry arrays that the emit fills much later: eh / rs and ew / lw (the two
// scans' inputs and outputs per position of the order), then pq over eh (per
// position: the position of that write; read by the entry flags).  Behind the
// marks, over the walk's arrays: gf / mf (per command: it is a Get; it is a
// miss) and their exclusive scans gslot / mslot.
struct AplWs {
  uint32_t *ans, *eh, *rs, *ew, *lw, *pq, *gf, *mf, *gslot, *mslot;
};

// The batch SSTable decode's arguments and scratch (lsmck_sstmerge.hip dec_*).
// Per table: segfirst (its hint's items, then their exclusive scan: its place
// in segpos; ntab + 1), state / fail (lsmck_sstmerge.hip kDec*; bit 0 of fail:
// a segment's landing did not check, bit 1: its spans were refused), lastcnt
// (its last segment's records), cons (the bytes its iterator got through),
// tabfirst (its entries, then their exclusive scan; ntab + 1), hint (its
// entries come from the segments).  segpos: nslots segment starts.  info: 5
// words -- [0] the first table refused (atomic min, set to ~0 by the caller),
// [1] the entries, [2] the tables whose index was refused (set to 0), [3] the
// segments, [4] the tables whose index was proven item by item (set to 0).
namespace mrg { struct OKey; }
struct DecArgs {
  const uint8_t *data, *index;  // index: null without a hint
  uint64_t data_bytes, index_bytes;
  const lsmck_sstable_span* spans;
  uint64_t ntab, nslots;
  uint64_t *segfirst, *segpos, *cons, *tabfirst, *bsum;
  uint32_t *state, *fail, *lastcnt;
  uint8_t* hint;
  unsigned long long* info;
};
// The batch merge's (mrg_*).  Per entry: ok (its order key), etab (its
// table), live (its live flag, then the flags' exclusive scan; n + 1), tomb
// (a tombstone winner to report).  tf / gf: table_first and group_first on
// the device; tgrp: every table's group; gout: the groups' first output
// entries (ngrp + 1).  mode: 0 report tombstone winners, 1 drop them, 2 keep
// them.  info: 3 words set to ~0 by the caller -- [0] the first entry refused
// (atomic min), [1] the live entries, [2] the first tombstone winner (its
// output slot << 32 | the entry; atomic min).
struct MrgArgs {
  const uint8_t *keys, *vals;
  uint64_t keys_bytes, vals_bytes;
  const lsmck_wal_cmd* ents;
  uint64_t n, ntab, ngrp;
  const uint64_t *tf, *gf;
  const uint32_t* tgrp;
  mrg::OKey* ok;
  uint32_t* etab;
  uint64_t *live, *gout, *bsum;
  uint8_t* tomb;
  uint32_t mode;
  unsigned long long* info;
};
// The batch point read's arguments and scratch (lsmck_sstget.hip get_*).  Per
// table: itemfirst (its index's items, then their exclusive scan: its place in
// the item arrays; ntab + 1), state (kGet*), fail (bit 0: an item of a
// one-length index was not where it was expected).  Per item slot (nslots):
// ioff (its offset in its index image), ipos (its position), iok (its order
// key).  Per query: qok (its order key), win (the lowest table that answered;
// LSMCK_GET_NONE: none yet).  count: the probe counts its pairs.  base: the
// number of table 0 as a source in win (0; lsmck_db_get_batch's runs come in
// front of the tables).  info: 5 words -- [0] the first table refused and [1]
// the first query refused (atomic min, set to ~0 by the caller), [2] the items
// of all tables, [3] the (query, table) pairs probed and [4] those whose
// interval was walked (set to 0).
struct GetArgs {
  const uint8_t *data, *index, *qkeys;
  uint64_t data_bytes, index_bytes, qkeys_bytes;
  const lsmck_sstable_span* spans;
  const lsmck_get_query* q;
  uint64_t ntab, n, nslots;
  uint64_t *itemfirst, *bsum, *ioff, *ipos;
  mrg::OKey *iok, *qok;
  uint32_t *state, *fail, *win;
  uint32_t count;
  unsigned long long* info;
  uint32_t base;
};
// The batch Db::get's (lsmck_dbget.hip dbg_*): the point read's arguments --
// g.base = nrun, g.info holding 10 words -- and the runs.  runs: the
// descriptors on the device; rf: the exclusive scan of their nent (nrun + 1);
// nent = rf[nrun]; rok: every run entry's order key.  Per query: res (the
// results, scratch until the error words are back), len (its answered length,
// then the lengths' exclusive scan; n + 1; null without a gather) and src (its
// value's address).  g.info[5] = the first run entry refused (atomic min, set
// to ~0 by the caller), [6] the queries a run answered (set to 0), [7] the
// gathered bytes, [8] the pairs an opened set's fences dropped (set to 0;
// lsmck_tableset.hip, whose table arrays lie in the set and not in scratch),
// [9] those its filters dropped behind the fences (set to 0).
namespace ts { struct Fence; }
namespace blm { struct Desc; }
struct DbArgs {
  GetArgs g;
  const lsmck_get_run* runs;
  const uint64_t* rf;
  uint64_t nrun, nent;
  mrg::OKey* rok;
  lsmck_get_result* res;
  uint64_t *len, *src;
};

}  // namespace lsmck

extern "C" {
// batch Db::get (lsmck_dbget.hip); the index pass and the table probe are the point read's
int lsmk_dbg_runs(const lsmck::DbArgs* a, hipStream_t st);     // the run entries' check, order keys, order (nent > 0)
int lsmk_dbg_probe(const lsmck::DbArgs* a, hipStream_t st);    // every (query, run) pair (n > 0, nent > 0)
int lsmk_dbg_resolve(const lsmck::DbArgs* a, hipStream_t st);  // res, len / src and the lengths' scan (n > 0)
int lsmk_dbg_gather(const lsmck::DbArgs* a, uint8_t* out, uint64_t total, hipStream_t st);
// batch point read (lsmck_sstget.hip)
int lsmk_get_index(const lsmck::GetArgs* a, hipStream_t st);  // spans, the map's parse, order, order keys (ntab > 0)
int lsmk_get_probe(const lsmck::GetArgs* a, hipStream_t st);  // the queries' check, then every (query, table) pair
// lsmk_get_probe's two halves, for lsmck_db_get_batch, whose run probe goes between them
int lsmk_get_queries(const lsmck::GetArgs* a, hipStream_t st);  // the queries' check, order keys, win = none (n > 0)
int lsmk_get_pairs(const lsmck::GetArgs* a, hipStream_t st);    // every (query, table) pair: a winner is a->base + t
int lsmk_get_resolve(const lsmck::GetArgs* a, lsmck_get_result* res, hipStream_t st);
// opened table set (lsmck_tableset.hip)
int lsmk_ts_fences(const lsmck::GetArgs* a, lsmck::ts::Fence* fence, uint32_t cap, hipStream_t st);  // behind lsmk_get_index
// lsmk_get_pairs behind the fences and, with desc, the filters (filt, and qh from lsmk_ts_hash; info[9] = the pairs they drop)
int lsmk_ts_pairs(const lsmck::GetArgs* a, const lsmck::ts::Fence* fence, const lsmck::blm::Desc* desc, const uint32_t* filt,
                  const uint64_t* qh, hipStream_t st);
// ... its filters ("bloom_bits" > 0; lanes = the set's items + its tables): count, sizes (info[5..7]), fill; a get's hashes
int lsmk_ts_bloom_count(const lsmck::GetArgs* a, uint64_t lanes, uint32_t cap, unsigned long long* nkeys, uint32_t* over,
                        hipStream_t st);
int lsmk_ts_bloom_size(uint64_t ntab, uint32_t bits, const unsigned long long* nkeys, const uint32_t* over,
                       lsmck::blm::Desc* desc, unsigned long long* info, hipStream_t st);
int lsmk_ts_bloom_fill(const lsmck::GetArgs* a, uint64_t lanes, uint32_t cap, const lsmck::blm::Desc* desc, uint32_t* filt,
                       hipStream_t st);
int lsmk_ts_hash(const lsmck::GetArgs* a, uint64_t* qh, hipStream_t st);
// batch SSTable decode and merge (lsmck_sstmerge.hip); ntab > 0 and n > 0
int lsmk_dec_index(const lsmck::DecArgs* a, hipStream_t st);     // spans, index parse, segment starts
int lsmk_dec_segments(const lsmck::DecArgs* a, hipStream_t st);  // the segments' check
int lsmk_dec_count(const lsmck::DecArgs* a, hipStream_t st);     // counts (plain walks) and their scan
int lsmk_dec_emit(const lsmck::DecArgs* a, lsmck_wal_cmd* ents, hipStream_t st);
int lsmk_mrg_keys(const lsmck::MrgArgs* a, hipStream_t st);    // validity, order keys, tables, key order
int lsmk_mrg_shadow(const lsmck::MrgArgs* a, hipStream_t st);  // live flags
int lsmk_mrg_scan(const lsmck::MrgArgs* a, hipStream_t st);    // their scan, the stuck word, the groups' firsts
int lsmk_mrg_place(const lsmck::MrgArgs* a, lsmck_wal_cmd* out, uint32_t* src, hipStream_t st);
// exclusive scan of v[0..n) in place, v[n] and *total = the sum (bsum: lsmk_sst_scan_blocks(n) + 1 entries)
int lsmk_sst_scan(uint64_t* v, uint64_t n, uint64_t* bsum, unsigned long long* total, hipStream_t st);
// batch memtable build (lsmck_memtable_build; lsmck_memtable.hip mem_*)
size_t lsmk_mem_carve(uint8_t* ws, uint64_t n, lsmck::MemWs* W);
int lsmk_mem_validate(const lsmck_wal_cmd* cmds, uint64_t n, uint64_t keys_bytes, uint64_t vals_bytes,
                      unsigned long long* info, hipStream_t st);
int lsmk_mem_init(const lsmck::MemWs* W, uint64_t n, hipStream_t st);
int lsmk_mem_chunk(const lsmck::MemWs* W, const uint8_t* keys, const lsmck_wal_cmd* cmds, uint64_t m, uint64_t r,
                   hipStream_t st);
int lsmk_mem_sort_regroup(const lsmck::MemWs* W, uint64_t m, uint64_t r, unsigned group_bits, void* tmp,
                          size_t* tmp_bytes, unsigned long long* count, hipStream_t st);
int lsmk_mem_resolve(const lsmck::MemWs* W, const lsmck_wal_cmd* cmds, uint64_t n, void* tmp, size_t* tmp_bytes,
                     unsigned long long* bytes, hipStream_t st);
int lsmk_mem_emit(const lsmck::MemWs* W, const lsmck_wal_cmd* cmds, uint64_t n, lsmck_wal_cmd* ents, uint32_t* src,
                  hipStream_t st);
int lsmk_mem_recs_to_cmds(const lsmck_wal_rec16* recs, uint64_t n, uint64_t img_bytes, lsmck_wal_cmd* cmds,
                          hipStream_t st);
// batch write plan (lsmck_db_write_plan; lsmck_writeplan.hip wpl_*)
void lsmk_wpl_carve(const lsmck::MemWs* W, lsmck::WplWs* P);
int lsmk_wpl_check(const lsmck_wal_cmd* cmds, uint64_t n, const uint8_t* tomb, unsigned long long* info,
                   hipStream_t st);
int lsmk_wpl_prep(const lsmck::WplWs* P, const lsmck_wal_cmd* cmds, uint64_t n, hipStream_t st);
int lsmk_wpl_walk(const lsmck::WplWs* P, uint64_t n, uint64_t limit, uint32_t cap, unsigned long long* steps,
                  hipStream_t st);
int lsmk_wpl_chain(const lsmck::WplWs* P, uint64_t n, uint32_t block, uint64_t limit, uint32_t* elist, uint32_t ecap,
                   uint32_t* bfirst, unsigned long long* cinfo, hipStream_t st);
int lsmk_wpl_mark(const lsmck::WplWs* P, uint64_t n, uint32_t block, const uint32_t* elist,
                  const unsigned long long* cinfo, const uint32_t* bfirst, void* tmp, size_t* tmp_bytes,
                  hipStream_t st);
int lsmk_wpl_emit(const lsmck::WplWs* P, const lsmck_wal_cmd* cmds, uint64_t n, uint64_t nent, uint64_t nseg,
                  int closed, uint64_t tomb_off, lsmck_wal_cmd* ents, uint32_t* src, lsmck_write_seg* segs, void* tmp,
                  size_t* tmp_bytes, hipStream_t st);
int lsmk_wpl_number(const lsmck::WplWs* P, uint64_t n, uint32_t block, const uint32_t* elist,
                    const unsigned long long* cinfo, const uint32_t* bfirst, void* tmp, size_t* tmp_bytes,
                    hipStream_t st);
// batch command stream (lsmck_db_apply_plan; lsmck_apply.hip apl_*): the four
// pieces that replace the write plan's where Gets stand between the writes.
// info: 9 words -- [0] the first command refused (atomic min, set to ~0 by the
// caller), [1] the tombstone byte is bad (set to 0), [7] the Gets, [8] the misses
// (written behind the slots' scans; [2..6] are the walk's and the chain's)
void lsmk_apl_carve(const lsmck::MemWs* W, const lsmck::WplWs* P, lsmck::AplWs* A);
int lsmk_apl_validate(const lsmck_wal_cmd* cmds, uint64_t n, uint64_t keys_bytes, uint64_t vals_bytes,
                      const uint8_t* tomb, unsigned long long* info, hipStream_t st);
// aw and mark, then prev, ans, pq and the writes as act (n + 1).  tmp == nullptr: *tmp_bytes alone
int lsmk_apl_prep(const lsmck::WplWs* P, const lsmck::AplWs* A, const lsmck_wal_cmd* cmds, uint64_t n, void* tmp,
                  size_t* tmp_bytes, hipStream_t st);
// behind lsmk_wpl_number: the entry flags and their slots (ex[n] = the entries), the Gets' and the misses' slots
int lsmk_apl_flag(const lsmck::WplWs* P, const lsmck::AplWs* A, uint64_t n, unsigned long long* info, void* tmp,
                  size_t* tmp_bytes, hipStream_t st);
// gets, and miss_q / miss_get (both or neither)
int lsmk_apl_gets(const lsmck::WplWs* P, const lsmck::AplWs* A, const lsmck_wal_cmd* cmds, const uint8_t* vals,
                  uint64_t n, uint64_t tomb_off, lsmck_apply_get* gets, lsmck_get_query* miss_q, uint32_t* miss_get,
                  hipStream_t st);
// segs[g] = {0, nent, 0}: an open segment, before the emit writes what it knows of it
int lsmk_apl_open_seg(lsmck_write_seg* segs, uint64_t g, uint64_t nent, hipStream_t st);
int lsmk_launch_crc32_fixed(const lsmck::CrcParams* P, int ncu, int variant, hipStream_t st);
int lsmk_launch_sha256(const lsmck::ShaParams* P, hipStream_t st);
int lsmk_launch_sha256_slices(const lsmck::ShaSliceParams* P, hipStream_t st);
uint64_t lsmk_walk_sb_count(uint64_t n);
int lsmk_launch_crc32_walk(const lsmck::CrcParams* P, uint64_t* sb_prefix, int ncu, int variant, hipStream_t st);
// stream kernel for sorted, non-overlapping batches (packed or with small gaps;
// a caller's batch is checked on the device unless `trusted`: P->sflag;
// P->sflag holds two u32, the flag and the slice tickets; P->scuts holds
// lsmk_stream_slices_max(ncu) + 1 entries)
uint32_t lsmk_stream_slices_max(int ncu);
int lsmk_ab_ablations(void);  // 1: built with -DLSMCK_AB_ABLATIONS (tools/build_ab.sh)
int lsmk_launch_crc32_stream(const lsmck::CrcParams* P, int ncu, int variant, int trusted, hipStream_t st);
uint64_t lsmk_wal_words(uint64_t n);
uint64_t lsmk_wal_scan_blocks(uint64_t n);
int lsmk_wal_mark_range(const uint8_t* img, uint64_t n, uint64_t b0, uint64_t b1, uint64_t* bits, uint32_t* pre,
                        hipStream_t st);
int lsmk_wal_mark(const uint8_t* img, uint64_t n, uint64_t* bits, uint32_t* pre, uint32_t* bsum, uint32_t* total,
                  int marked, uint64_t w0, uint64_t w1, hipStream_t st);
int lsmk_wal_chain(const uint8_t* img, uint64_t n, const uint64_t* bits, const uint32_t* pre, uint32_t nc, int levels,
                   uint64_t* pos, uint32_t* J, uint64_t* badpos, uint32_t* chain, unsigned long long* info, uint64_t w0,
                   uint64_t w1, uint64_t start, uint64_t lim, hipStream_t st);
int lsmk_wal_frame_insert(uint8_t* img, const uint64_t* off, const uint32_t* len, const uint32_t* crc, uint64_t n,
                          uint32_t kmax, hipStream_t st);
// batch WAL encode (lsmck_wal_encode_batch; lsmck_wal.hip wal_encode_*)
static_assert(sizeof(lsmck_wal_cmd) == 32, "lsmck_wal_cmd is 32 bytes");
uint32_t lsmk_wal_encode_tile(void);            // the gather's tile bytes
uint64_t lsmk_wal_encode_scan_blocks(uint64_t n);  // bsum entries of the offset scan
// sizes, validation and the exclusive scan: off[0..n] (off[n] = the total);
// info[0] = the first invalid command (atomic min; the caller sets it to ~0),
// info[1] = the total
int lsmk_wal_encode_scan(const lsmck_wal_cmd* cmds, uint64_t n, uint64_t keys_bytes, uint64_t vals_bytes,
                         uint64_t* off, uint64_t* bsum, unsigned long long* info, hipStream_t st);
// the image but its CRC fields (zero bytes) from the arenas and the commands
int lsmk_wal_encode_gather(const uint8_t* keys, const uint8_t* vals, const lsmck_wal_cmd* cmds, uint64_t n,
                           const uint64_t* off, uint8_t* img, uint64_t total, hipStream_t st);
// payload descriptors for the CRC batch
int lsmk_wal_encode_desc(const lsmck_wal_cmd* cmds, uint64_t n, const uint64_t* off, uint64_t* poff, uint32_t* plen,
                         hipStream_t st);
// the records' CRC fields
int lsmk_wal_encode_stamp(uint8_t* img, const uint64_t* off, const uint32_t* crc, uint64_t n, hipStream_t st);
// the exclusive scan of nb u64 block sums in place (wal_seg_scan_b alone)
int lsmk_scan_u64_blocks(uint64_t* bsum, uint32_t nb, hipStream_t st);
// batch SSTable encode (lsmck_sstable_encode_batch; lsmck_sstable.hip sst_*).
// info: 4 words the caller sets to ~0 -- [0] the first invalid entry (atomic
// min), [1] the data arena's bytes, [2] the first table too long to hash
// (atomic min), [3] the index arena's bytes
uint32_t lsmk_sst_tile(void);                // the gather's tile bytes
uint64_t lsmk_sst_scan_blocks(uint64_t n);   // bsum entries of a scan over n values
// sizes, validation and the exclusive scan: off[0..n]
int lsmk_sst_sizes(const lsmck_wal_cmd* ents, uint64_t n, uint64_t keys_bytes, uint64_t vals_bytes, uint64_t* off,
                   uint64_t* bsum, unsigned long long* info, hipStream_t st);
// key order inside every table (first: n bytes, zeroed by the caller; tf: ntab + 1 on the device)
int lsmk_sst_order(const lsmck_wal_cmd* ents, uint64_t n, const uint8_t* keys, uint64_t keys_bytes,
                   uint64_t vals_bytes, const uint64_t* tf, uint64_t ntab, uint8_t* first, unsigned long long* info,
                   hipStream_t st);
// the index items' sizes and their scan: ioff[0..nitems]
int lsmk_sst_index_plan(const uint32_t* item_ent, uint64_t nitems, const lsmck_wal_cmd* ents, uint64_t* ioff,
                        uint64_t* bsum, unsigned long long* info, hipStream_t st);
// spans and the digests' descriptors per table; hash: bit 0 the data images are hashed, bit 1 the index images
int lsmk_sst_spans(const uint64_t* tf, const uint64_t* ibase, uint64_t ntab, const uint64_t* off, const uint64_t* ioff,
                   lsmck_sstable_span* spans, uint64_t* doff, uint32_t* dlen, uint64_t* xoff, uint32_t* xlen,
                   unsigned hash, unsigned long long* info, hipStream_t st);
int lsmk_sst_gather(const uint8_t* keys, const uint8_t* vals, const lsmck_wal_cmd* ents, uint64_t n,
                    const uint64_t* off, uint8_t* img, uint64_t total, hipStream_t st);
int lsmk_sst_index_write(const uint32_t* item_tab, const uint32_t* item_ent, uint64_t nitems, const uint64_t* tf,
                         const lsmck_wal_cmd* ents, const uint8_t* keys, const uint64_t* off, const uint64_t* ioff,
                         uint8_t* index, hipStream_t st);
int lsmk_wal_emit(const uint8_t* img, uint64_t n, const uint32_t* chain, const uint64_t* pos,
                  const unsigned long long* info, uint32_t m, lsmck_wal_rec* recs, uint64_t* poff, uint32_t* plen,
                  uint32_t* pcrc, hipStream_t st);
// the segment walk (lsmck_segwalk.h; lsmck_wal.hip wal_seg_*)
namespace lsmck { namespace seg { struct SegArgs; } }
uint64_t lsmk_wal_seg_bytes(uint64_t len, uint64_t want);
uint64_t lsmk_wal_seg_scan_blocks(uint32_t K);
int lsmk_wal_seg_walk(const lsmck::seg::SegArgs* a, hipStream_t st);
int lsmk_wal_seg_round(const lsmck::seg::SegArgs* a, uint64_t* bsum, hipStream_t st);
int lsmk_wal_seg_repair(const lsmck::seg::SegArgs* a, uint32_t budget, hipStream_t st);
// a parallel repair round (seg::seg_prepair): g0 / x0 / code0 hold K entries (the snapshot)
int lsmk_wal_seg_prepair(const lsmck::seg::SegArgs* a, uint64_t* g0, uint64_t* x0, uint32_t* code0, hipStream_t st);
// recs: lsmck_wal_rec[] or, compact != 0, lsmck_wal_rec16[]
int lsmk_wal_seg_emit(const lsmck::seg::SegArgs* a, uint64_t at, void* recs, int compact, uint64_t* poff,
                      uint32_t* plen, uint32_t* pcrc, hipStream_t st);
int lsmk_wal_seg_emit_packed(const lsmck::seg::SegArgs* a, uint64_t at, void* recs, int compact, uint64_t* poff,
                             uint32_t* plen, uint32_t* pcrc, uint64_t iend, hipStream_t st);
int lsmk_wal_seg_place(const lsmck::seg::SegArgs* a, uint64_t at, void* recs, int compact, uint64_t* poff,
                       uint32_t* plen, uint32_t* pcrc, uint64_t iend, int packed, hipStream_t st);
// m wide records -> lsmck_wal_rec16 (out)
int lsmk_wal_recs_compact(const lsmck_wal_rec* in, void* out, uint64_t m, hipStream_t st);
int lsmk_launch_crc32_compare(const uint32_t* crc, const uint32_t* expected, uint64_t n,
                               unsigned long long* n_bad, unsigned long long* first_bad, hipStream_t st);
int lsmk_sha_order(const uint32_t* len, size_t n, uint16_t* keys_out, uint32_t* order, void* tmp, size_t* tmp_bytes,
                   int coarse, int from, hipStream_t st);
int lsmk_sha_split(const uint16_t* keys, size_t n, uint32_t t, uint64_t* split, hipStream_t st);
int lsmk_launch_gen_stream(unsigned char* dst, uint64_t seed, uint64_t byte_off, uint64_t n, hipStream_t st);
}
#endif
