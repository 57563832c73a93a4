/*
 * lsmck.h -- C ABI of liblsmck.so, the MI355X-native checksum path of the
 * lsm_storage_engine reference (myroslavlisniak/lsm_storage_engine).
 *
 * The reference has no plugin/FFI API; its checksum path sits behind two Rust
 * seams:
 *   (i)  crc::crc32::checksum_ieee(&[u8]) -> u32, crate `crc` ^1.7
 *        (Cargo.toml:14), called at src/wal.rs:135,153 (replay verify) and
 *        src/wal.rs:177,187 (append);
 *   (ii) the crate-private Checksums API of src/checksums.rs:
 *        calculate_checksum (:20-38), verify (:40-62), write_checksums (:64-80),
 *        called from src/sync/sstable.rs:119,139,210 and
 *        src/tokio/sstable.rs:34,88,189.
 * Every entry point below names the reference item it replaces.  The Rust
 * bindings a maintainer would add are in INTEGRATION.md.
 *
 * Conventions
 *   - Plain pointers and sizes only.  The caller owns every buffer; the library
 *     never retains a caller pointer after the call returns (synchronous calls)
 *     or after the work on `stream` completes (LSMCK_DEVICE calls).
 *   - Return values: 0 = ok; < 0 = error (-EINVAL, -ENOMEM, -EIO, or
 *     LSMCK_EHIP - hipError_t); > 0 = an integrity verdict documented at the
 *     function.  lsmck_last_error() holds a thread-local message.
 *   - Scalar entry points (section 1) run on the calling CPU thread.  They are
 *     the per-record latency path (one WAL append = one call; a kernel launch
 *     costs microseconds), are reentrant and keep no mutable global state.
 *   - Batch entry points (section 3) run on the GPU and FAIL (return
 *     LSMCK_ENODEV) when no GPU / HIP runtime is usable: there is no CPU
 *     fallback for a batch.
 */
#ifndef LSMCK_H
#define LSMCK_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSMCK_ABI_VERSION 1

/* error codes (negative) */
#define LSMCK_EINVAL (-22)
#define LSMCK_ENOMEM (-12)
#define LSMCK_EIO (-5)
#define LSMCK_ENODEV (-19)
#define LSMCK_ENOSPC (-28) /* the batch builders (encode, build, decode, merge): an output buffer is too small */
#define LSMCK_EHIP (-1000) /* LSMCK_EHIP - hipError_t */

/* flags for batch calls */
#define LSMCK_DEVICE 0x1u      /* base/off/len/out are device pointers; async on `stream` */
#define LSMCK_HOST 0x0u        /* host (pageable) pointers; staged through pinned memory; synchronous */
#define LSMCK_HOST_PINNED 0x2u /* host pointers already pinned (hipHostMalloc); DMA without a copy */
/* with LSMCK_DEVICE, descriptor CRC batches only: the caller asserts that its
 * records are sorted by offset, do not overlap, and that every byte between
 * the first record's start and the last record's end lies in memory it may
 * read (one buffer, e.g. a WAL image or a data file).  The stream kernel then
 * takes the batch without the device-side check of its descriptors (one pass
 * over them; lsmck_wal_replay_verify does the same for its own payloads). */
#define LSMCK_SORTED 0x4u

/* ======================================================================== */
/* 1. Scalar CPU entry points                                                */
/* ======================================================================== */

/* Replaces crc::crc32::checksum_ieee (crc ^1.7) at src/wal.rs:135,153,177,187.
 * CRC-32/ISO-HDLC: reflected 0xEDB88320, init/xorout 0xFFFFFFFF.
 * n == 0 accepts any p (an empty Rust slice passes a dangling non-null pointer)
 * and returns 0. */
uint32_t lsmck_crc32_ieee(const uint8_t* p, size_t n);

/* crc of (A || B) from crc(A) and the bytes of B (zlib crc32() convention);
 * lsmck_crc32_update(0, p, n) == lsmck_crc32_ieee(p, n). */
uint32_t lsmck_crc32_update(uint32_t crc_a, const uint8_t* p, size_t n);

/* crc of (A || B) from crc(A), crc(B) and |B|. */
uint32_t lsmck_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* SHA-256 (sha2 ^0.10.1 Sha256, src/checksums.rs:21,34,36). */
typedef struct {
  uint32_t h[8];
  uint64_t nbytes;
  uint8_t buf[64];
  uint32_t nbuf;
} lsmck_sha256_ctx;
void lsmck_sha256_init(lsmck_sha256_ctx* c);
void lsmck_sha256_update(lsmck_sha256_ctx* c, const uint8_t* p, size_t n);
void lsmck_sha256_final(lsmck_sha256_ctx* c, uint8_t out[32]);
void lsmck_sha256(const uint8_t* p, size_t n, uint8_t out[32]);

/* base64 ^0.13 `encode` (STANDARD alphabet, '=' padded), src/checksums.rs:37.
 * Writes 4*ceil(n/3) chars plus a NUL; returns the char count. */
size_t lsmck_base64_encode(const uint8_t* p, size_t n, char* out);

/* Positive status codes mark the places where the reference PANICS; negative
 * ones (-errno, LSMCK_EJSON) the places where it returns Err(io::Error).
 *   LSMCK_PANIC_OPEN_FILE      calculate_checksum's .expect("Can't open file to
 *                              calculate checksum") (src/checksums.rs:22-25), on the
 *                              file given (lsmck_checksum_file) or on the data file
 *                              (verify / write_checksums: it is hashed first, :41, :65)
 *   LSMCK_PANIC_OPEN_INDEX     the same panic on the index file (:42, :66)
 *   LSMCK_PANIC_OPEN_CHECKSUM  verify's .expect("Can't open checksum file") (:43-46)
 * A read error after a successful open is -errno (the `?` at :30). */
#define LSMCK_PANIC_OPEN_FILE 4
#define LSMCK_PANIC_OPEN_INDEX 5
#define LSMCK_PANIC_OPEN_CHECKSUM 6

/* Replaces Checksums::calculate_checksum(path) (src/checksums.rs:20-38):
 * SHA-256 of the whole file, base64 -> out (44 chars + NUL).  Returns 0,
 * LSMCK_PANIC_OPEN_FILE when the file cannot be opened (the reference panics,
 * :25), or -errno on a read error (Err, :30). */
int lsmck_checksum_file(const char* path, char out[45]);

/* Replaces Checksums::write_checksums(&SsTableMetadata) (src/checksums.rs:64-80):
 * hashes the data and index files and writes
 * {"index_checksum":"<b64>","data_checksum":"<b64>"} to checksum_path, opened
 * write+create WITHOUT truncate exactly as the reference opens it (:75-78).
 * Returns 0, LSMCK_PANIC_OPEN_FILE / LSMCK_PANIC_OPEN_INDEX (a data / index
 * file cannot be opened: panic), or -errno (a read error, or the checksum
 * file cannot be opened or written: Err, :78-79). */
int lsmck_checksums_write(const char* data_path, const char* index_path, const char* checksum_path);

/* Replaces Checksums::verify(&SsTableMetadata) (src/checksums.rs:40-62).
 * Returns, in the reference's order of checks:
 *   LSMCK_PANIC_OPEN_FILE / -errno      data file: cannot be opened (panic) / read error (Err)
 *   LSMCK_PANIC_OPEN_INDEX / -errno     index file: the same
 *   LSMCK_PANIC_OPEN_CHECKSUM           checksum file cannot be opened (panic, :46)
 *   LSMCK_EJSON / -errno                checksum file is not JSON of the Checksums
 *                                       shape, or cannot be read (Err, :48)
 *   LSMCK_DATA_MISMATCH / LSMCK_INDEX_MISMATCH   digest mismatch (panic, :49-60;
 *                                       data is checked first)
 *   0                                   both digests match */
#define LSMCK_DATA_MISMATCH 1
#define LSMCK_INDEX_MISMATCH 2
#define LSMCK_EJSON (-74)
int lsmck_checksums_verify(const char* data_path, const char* index_path, const char* checksum_path);

/* WAL record framing, CommandLog::log (src/wal.rs:165-196).
 * Insert: [u8 1][u32 crc LE][u32 klen][u32 vlen][key][val], crc over key||val.
 * Remove: [u8 2][u32 crc LE][u32 klen][key], crc over key.
 * Return the record size (13+klen+vlen / 9+klen); out must hold that much. */
size_t lsmck_wal_encode_insert(const uint8_t* key, uint32_t klen, const uint8_t* val, uint32_t vlen,
                               uint8_t* out);
size_t lsmck_wal_encode_remove(const uint8_t* key, uint32_t klen, uint8_t* out);

/* ======================================================================== */
/* 2. Device context                                                          */
/* ======================================================================== */
typedef struct lsmck_ctx lsmck_ctx;

/* Binds a context to HIP device `device` (one context per GPU; thread-safe:
 * concurrent calls on one context are serialised on its scratch). NULL on
 * failure (see lsmck_last_error). */
lsmck_ctx* lsmck_ctx_create(int device);
void lsmck_ctx_destroy(lsmck_ctx* ctx);
const char* lsmck_last_error(void);
int lsmck_device_count(void);

/* Tuning knobs of a context (no effect on results, only on speed):
 *   "crc_stream"  descriptor CRC batches: 1 = the stream kernel for sorted
 *                 batches (default), 0 = the walking kernel only (A/B),
 *                 2 = the stream kernel only (DIAGNOSTIC: a caller batch it
 *                 declines gets no CRCs).
 *   "crc_ablate"  DIAGNOSTIC ONLY, results are invalid while set: 3 = payload
 *                 loads only (ring, stream and walking kernels: the bench's
 *                 loads-only ceiling); 0 = off.  2 (the stream kernel without
 *                 payload loads) and 4..12 (stream kernel ablations,
 *                 DESIGN.md 3.1 items 10-11) only in A/B builds
 *                 (-DLSMCK_AB_ABLATIONS, tools/build_ab.sh).
 *   "sha_order"   variable-length SHA-256 batches of >= 2048 messages run in
 *                 decreasing length order (1, default) or batch order (0).
 *                 A/B switch; digests are identical either way.
 *   "sha_bucket_shift" / "sha_bucket_from"  that order's length key: messages
 *                 of from..1023 compression blocks share a bucket per
 *                 2^shift blocks (defaults 2 and 128; shift 0 = exact block
 *                 counts).  A/B switch; digests are identical either way.
 *   "sha_short_blocks"  in that order, messages of at most this many
 *                 compression blocks run on a lean kernel with more waves per
 *                 SIMD (default 12; 0 = every message on the window kernel).
 *                 Digests are identical either way.
 *   "sha_pair"    the window kernel loads two blocks (a 128-B line) per window
 *                 (1, default) or one (0); 2 and 3 are diagnostics (no payload
 *                 loads: digests invalid / line-aligned loads realigned
 *                 through LDS).
 *   "tree_active_files" / "tree_slice_bytes"  lsmck_checksums_verify_many's
 *                 files in flight (0 = 8192) and bytes of a file per round
 *                 (0 = 128 KiB; a multiple of 64).  Tests use small values.
 *   "tree_list_threads"  lsmck_tree_verify's metadata parsing threads (0 = 8).
 *   "tree_cpu_file_bytes"  whole-tree verify: files of at least this many
 *                 bytes are hashed on 4 host threads (SHA-NI where present)
 *                 instead of a GPU lane (0 = 16 MiB).
 *   "wal_prefetch"  bytes lsmck_wal_replay_verify's header walk prefetches
 *                 ahead of its position (default 4096; 0 = off).  A/B switch.
 *   "stage_numa"  where host-memory batches stage: -2 (default) the
 *                 device's NUMA node when the host has several -- pinned
 *                 buffers allocated there (lsmck_host_alloc_pinned too) and the
 *                 copy threads on its CPUs; -1 HIP's default placement and
 *                 unpinned threads; >= 0 that node.  Applies to buffers
 *                 allocated after the call.
 *   "stage_threads"  host-memory batches: threads that copy a pageable chunk
 *                 into its pinned staging slot (default 8; 1 = one memcpy).
 *   "wal_gpu_walk"  lsmck_wal_replay_verify of a device image: 1 = header walk
 *                 on the GPU (default), 0 = read back and walk on the host.
 *   "wal_upload_min"  host images of at least this many bytes are uploaded and
 *                 walked on the GPU (default 1 MiB; 0 = always the host walk).
 *   "wal_split"   an uploaded host image is walked in two parts, the first
 *                 behind the upload of the second (1, default; taken when each
 *                 half holds one "wal_stage_bytes" chunk), or whole after it (0).
 *   "wal_stage_bytes"  an uploaded host WAL image moves in chunks of this many
 *                 bytes (pageable: copied into a pinned slot, then DMA'd; each
 *                 chunk's candidate marking runs behind its DMA); a multiple
 *                 of 64 KiB in [1 MiB, 64 MiB], default 16 MiB.
 *   "wal_register"  1 = an uploaded host WAL image is DMA'd from the caller's
 *                 own pages, pinned in place for the call (hipHostRegister),
 *                 instead of through the pinned staging copy (default 0).  A/B.
 *   "wal_chunk_bytes"  lsmck_wal_replay_verify of a host image: CRC batches
 *                 of this many payload bytes run on a helper thread while the
 *                 walk goes on (default 32 MiB; 0 = one batch after the walk).
 *   "tree_overlap"  lsmck_tree_verify reads the highest level's directory
 *                 first and, when it holds at least this many tables (default
 *                 2048; 0 = never), verifies them while the lower levels are
 *                 listed -- its first 8x this many as soon as they are
 *                 parsed, the rest once the level is read -- then the lower
 *                 levels' tables.  The report is the same either way (the
 *                 first failure in read_dir order).
 *   "tree_list_batch"  lsmck_tree_verify: metadata names per listing batch
 *                 (0 = 1024).  Tests use small values.
 *   "tree_json_threads"  whole-tree verify: threads reading the tables'
 *                 checksum files beside the stream (0 = default: 2, or 4 for
 *                 a batch of 16k tables or more).
 *   "tree_stages"  whole-tree verify: pinned slots its rounds cycle through
 *                 (3, default: a round is read while the two before it upload
 *                 and hash; 2 = round 4's double buffering).  A/B.
 *   "tree_open_files"  files kept open from their first slice to their last
 *                 (-1 = default: as many as RLIMIT_NOFILE leaves after a
 *                 1024-descriptor reserve; the rest reopen per slice).
 *   "wal_part_bytes"  the candidate-doubling GPU walk goes in parts of this
 *                 many bytes (0 = whole, default; otherwise >= 1 MiB; a
 *                 nonzero value also skips the segment walk).  Tests / A/B.
 *   "wal_seg_walk"  the GPU header walk: 1 = the segment walk (default;
 *                 lsmck_segwalk.h), falling back to candidate doubling when
 *                 its check keeps failing; 0 = candidate doubling only.
 *   "wal_seg_bytes"  segment walk: bytes per segment (0 = auto, default:
 *                 ~2^16 segments; else 64..2^30).  Tests use small segments.
 *   "wal_seg_rounds"  segment walk: check failures repaired before it
 *                 declines to candidate doubling (default 16).
 *   "wal_seg_prepair"  segment walk: parallel repair rounds (every segment
 *                 walked again from its predecessor's exit at once) after a
 *                 check with several failures, before the serial repairs
 *                 (default 2; 0 = none).
 *   "wal_seg_pack"  segment walk: 1 = the CRC pass runs over packed spans,
 *                 each payload with the next record's header, the header
 *                 then taken back out of the CRC (default); 0 = over the
 *                 payloads alone.  A/B; results are the same.
 *   "wal_seg_stage"  segment walk: the walk stages the records it passes so
 *                 they need no second walk of the headers: 1 = auto slots
 *                 per segment (default), 0 = off (A/B), N >= 2 = N slots
 *                 (tests).  A segment with more records is walked again.
 *   "wal_dma_engines"  device replays whose records go to the host: the
 *                 read-back is dealt over this many SDMA engines through HSA
 *                 (default 4; 1..16), beside the CRC pass and off the compute
 *                 units; 0 = hipMemcpyAsync on a staging stream (A/B).
 *   "wal_dma_chunks"  ... cut in this many pieces (default 32; 1..64); a
 *                 pageable records array is filled piece by piece as they land.
 *   "wal_pipe"    device replays of at least "wal_pipe_min" bytes (default
 *                 1 GiB): the log is walked in this many parts (2..64) on a
 *                 CU-masked stream while the previous part's CRC pass runs
 *                 on the other CUs; 0 or 1 = off (default 0: measured slower,
 *                 DESIGN.md 8).  "wal_pipe_first" the first part in 64ths
 *                 of the log (1..63, default 4), "wal_pipe_cus" the walk's
 *                 CUs (default 32), "wal_pipe_layout" which ones (0 the last,
 *                 1 spread), "wal_pipe_seg" the parts' segment bytes (0 =
 *                 sized to the walk's CUs).  A/B; results are the same.
 *   "wal_pipe_min"  the smallest log the pipeline takes, in bytes (>= 0).
 *   "tree_readers"  whole-tree verify: reader threads per context (default
 *                 16; 1..64).  A/B.
 *   "wal_encode_time"  DIAGNOSTIC, not part of the stable option list (it and
 *                 its stats may change or go with the tool that uses them):
 *                 1 = lsmck_wal_encode_batch records device events around
 *                 its stages (tools/wal_encode_big.py reads them back as
 *                 stats); 0 = none (default).
 *   "sst_encode_time"  DIAGNOSTIC, not part of the stable option list, as
 *                 "wal_encode_time": 1 = lsmck_sstable_encode_batch records
 *                 device events around its stages (tools/sst_encode_big.py
 *                 reads them back as stats); 0 = none (default).  It times
 *                 lsmck_sstable_decode_batch and lsmck_sstable_merge_batch
 *                 the same way (tools/merge_big.py), and
 *                 lsmck_sstable_get_batch (tools/get_big.py) and
 *                 lsmck_db_get_batch (tools/db_get_big.py), whose probes
 *                 then also count their pairs.
 *   "mem_build_time"  DIAGNOSTIC, not part of the stable option list, as
 *                 "wal_encode_time": 1 = lsmck_memtable_build records device
 *                 events around its stages (tools/memtable_big.py reads them
 *                 back as stats); 0 = none (default).  It times
 *                 lsmck_db_write_plan the same way (tools/write_big.py).
 *   "cut_walk_cap"  lsmck_db_write_plan: the commands a candidate start's
 *                 walk follows at most (default 4096, from 1); a memtable
 *                 longer than that is found by one workgroup on the chain.
 *   "cut_block"   lsmck_db_write_plan: the candidate starts one workgroup
 *                 links in LDS, 4 bytes each (default 8192; 64..8192).
 *   "fence_walk_cap"  lsmck_tableset_open: the records a fence's walk visits
 *                 at most (default 256, 1..2^20; INDEX_STEP is 100 and an
 *                 interval with one item missing 200).  Read when a set is
 *                 opened; a longer head or tail leaves that fence invalid.
 *   "bloom_bits"  lsmck_tableset_open: the bits per key of a resident bloom
 *                 filter per table (default 0: no filters; 4..64).  Read when
 *                 a set is opened, as "fence_walk_cap" is, whose cap the
 *                 filters' walks share; lsmck_ctx_get_stat("bloom_bits") is
 *                 the value in effect.  No result of any call depends on it.
 * Returns 0, or LSMCK_EINVAL for an unknown key / value. */
int lsmck_ctx_set_option(lsmck_ctx* ctx, const char* key, long value);

/* What the context's last call of a kind did (diagnostics for tests and
 * tools; no effect on results):
 *   "wal_walk_path"  the last lsmck_wal_replay_verify that walked on the GPU
 *                    or the host: 1 = segment walk, 2 = candidate doubling,
 *                    3 = host walk.
 *   "wal_seg_repairs"  its segment walk's repaired check failures.
 *   "wal_segments"   its segment walk's segment count.
 *   "wal_seg_prepairs"  its segment walk's parallel repair rounds.
 *   "wal_recs_dma"   its records' read-back to the host: the SDMA engines it
 *                    was dealt over, 0 = hipMemcpyAsync (or none read back).
 *   "wal_pipe_parts"  its pipelined parts ("wal_pipe"; 0 = one walk, one pass).
 *   "numa_node"      the device's NUMA node (sysfs of its PCI function; -1
 *                    unknown), and "stage_numa_node" the node the context's
 *                    pinned buffers and copy threads are placed on (-1: none).
 *   "wal_encode_tile"  bytes of the image one workgroup of lsmck_wal_encode_batch's
 *                    gather kernel writes (a power of two, at most 64 KiB;
 *                    tiles are aligned on the image's address).
 *   "wal_encode_scan_ns", "wal_encode_gather_ns", "wal_encode_crc_ns",
 *   "wal_encode_stamp_ns"  DIAGNOSTIC, subject to change: the last lsmck_wal_encode_batch's stages between
 *                    device events, with "wal_encode_time" 1: the size /
 *                    validate / scan kernels, the gather, the descriptors and
 *                    the CRC pass, the stamp.
 *   "sst_encode_tile"  bytes of the data arena one workgroup of
 *                    lsmck_sstable_encode_batch's gather kernel writes (a power
 *                    of two, at most 32 KiB; tiles are aligned on the arena's address).
 *   "sst_encode_scan_ns", "sst_encode_gather_ns", "sst_encode_index_ns",
 *   "sst_encode_sha_ns"  DIAGNOSTIC, subject to change: the last lsmck_sstable_encode_batch's
 *                    stages between device events, with "sst_encode_time" 1:
 *                    sizes / order / index plan / spans, the data gather, the
 *                    index writer, the two digest passes.
 *   "sst_decode_declined"  the tables of the last lsmck_sstable_decode_batch
 *                    whose index file was given and refused as a hint (they
 *                    were walked by one lane; the entries are the same).
 *   "sst_decode_uniform"  ... whose index file holds keys of one length: its
 *                    items lie a fixed step apart and were proven in place by
 *                    a thread each, without the serial parse.
 *   "sst_decode_index_ns", "sst_decode_seg_ns", "sst_decode_scan_ns",
 *   "sst_decode_emit_ns"  DIAGNOSTIC, subject to change: the last
 *                    lsmck_sstable_decode_batch's stages, with
 *                    "sst_encode_time" 1: the index walk, the segment walks,
 *                    the counts (plain walks included) and their scan, the
 *                    entries.
 *   "sst_merge_okey_ns", "sst_merge_shadow_ns", "sst_merge_scan_ns",
 *   "sst_merge_place_ns"  DIAGNOSTIC, subject to change: the last
 *                    lsmck_sstable_merge_batch's stages, with
 *                    "sst_encode_time" 1: validation and order keys, shadow,
 *                    the scan, place.
 *   "sst_get_index_ns", "sst_get_probe_ns", "sst_get_resolve_ns"
 *                    DIAGNOSTIC, subject to change: the last
 *                    lsmck_sstable_get_batch's stages, with "sst_encode_time"
 *                    1: the index pass, the queries' check and the probe of
 *                    every (query, table) pair, resolve; and
 *                    "sst_get_probed" / "sst_get_walked", the pairs that
 *                    probe looked up (the others were skipped behind a lower
 *                    table's answer) and those whose interval it walked.
 *   "db_get_runs_ns", "db_get_index_ns", "db_get_run_probe_ns",
 *   "db_get_probe_ns", "db_get_resolve_ns", "db_get_gather_ns"
 *                    DIAGNOSTIC, subject to change: the last
 *                    lsmck_db_get_batch's stages, with "sst_encode_time" 1:
 *                    the run pass, the index pass, the queries' check and the
 *                    probe of every (query, run) pair, the table probe,
 *                    resolve and the lengths' scan, the gather; and
 *                    "db_get_probed" / "db_get_walked", the (query, table)
 *                    pairs its table probe looked up and those whose interval
 *                    it walked, and "db_get_run_hits", the queries a run
 *                    answered.
 *   "mem_rounds"     the chunk rounds the last lsmck_memtable_build ran (0 for
 *                    fewer than two commands; each round is a host round trip).
 *   "mem_validate_ns", "mem_chunk_ns", "mem_sort_ns", "mem_resolve_ns"
 *                    DIAGNOSTIC, subject to change: the last
 *                    lsmck_memtable_build's stages between device events, with
 *                    "mem_build_time" 1: validate; the kernel that reads key
 *                    bytes, summed over the rounds; the rounds' fixed-width
 *                    part (sort passes, regroup, compaction), summed; resolve
 *                    and emit.
 *   "cut_steps"      the walk steps of the last lsmck_db_write_plan, summed
 *                    over the candidate starts (at most n * "cut_walk_cap");
 *                    "cut_long" the memtables longer than "cut_walk_cap" that
 *                    its chain resolved; "mem_rounds" is its order's rounds.
 *   "write_order_ns", "write_walk_ns", "write_chain_ns", "write_mark_ns",
 *   "write_emit_ns"  DIAGNOSTIC, subject to change: the last
 *                    lsmck_db_write_plan's stages between device events, with
 *                    "mem_build_time" 1: validation, the order's rounds and
 *                    prev; the walk; the blocks' exits and the chain; the
 *                    marks, the segment numbers and the entry flags; the sort
 *                    by segment and the outputs.
 *   "apply_gets", "apply_misses"  the Gets of the last lsmck_db_apply_plan and
 *                    those no write of its stream answers (the three keys
 *                    above are set by it as well).
 *   "apply_order_ns", "apply_prep_ns", "apply_walk_ns", "apply_chain_ns",
 *   "apply_mark_ns", "apply_emit_ns"  DIAGNOSTIC, subject to change: the last
 *                    lsmck_db_apply_plan's stages, with "mem_build_time" 1
 *                    (named at that call).
 * Returns 0 and *value, or LSMCK_EINVAL for an unknown key. */
int lsmck_ctx_get_stat(lsmck_ctx* ctx, const char* key, long* value);

/* ======================================================================== */
/* 3. Batch GPU entry points                                                  */
/* ======================================================================== */

/* CRC-32 of n records: record i = base[off[i] .. off[i]+len[i]).  The batch
 * form of checksum_ieee for WAL replay / bulk append (src/wal.rs:135,153,177).
 * Any offsets, lengths and order; every uint32_t length is supported, up to
 * 2^32-1 bytes a record (here, in lsmck_crc32_batch_fixed and in
 * lsmck_crc32_verify_batch; tests/test_gpu_crc_long.py).  A descriptor record
 * is one wave's work, however small the batch: a 4 GiB record measured 0.69 s
 * on the stream kernel and 1.5 s on the walking kernel (the fixed-size entry
 * point spreads a record over the chip: 6 ms).
 * A device batch whose records are sorted,
 * do not overlap, lie at most 64 bytes apart (a WAL's 13- / 9-byte headers)
 * and whose empty records sit at their predecessor's end runs on the stream
 * kernel (decided on the device, nothing read back); any other batch on the
 * walking kernel.  Host batches are staged in order and always take the
 * stream kernel.  stream: hipStream_t (NULL = the context's default stream). */
int lsmck_crc32_batch(lsmck_ctx* ctx, const uint8_t* base, const uint64_t* off, const uint32_t* len, size_t n,
                      uint32_t* out, unsigned flags, void* stream);

/* Fixed-size records: record i = base[i*stride .. i*stride+len).  Any stride:
 * with stride < len the records overlap (their shared bytes are read again). */
int lsmck_crc32_batch_fixed(lsmck_ctx* ctx, const uint8_t* base, size_t stride, uint32_t len, size_t n,
                            uint32_t* out, unsigned flags, void* stream);

/* Verify: compares against expected[i].  Host-visible results: *n_bad and
 * *first_bad (index of the first mismatching record in batch order, or n).
 * Synchronous.  Returns 0 when every record matches, 1 otherwise. */
int lsmck_crc32_verify_batch(lsmck_ctx* ctx, const uint8_t* base, const uint64_t* off, const uint32_t* len,
                             const uint32_t* expected, size_t n, unsigned flags, void* stream, uint64_t* n_bad,
                             uint64_t* first_bad);

/* SHA-256 of n messages -> out32[32*i .. 32*i+32).  The batch form of
 * calculate_checksum's digest (src/checksums.rs:20-38).  Messages may lie in
 * any order, overlap and repeat.  Fixed form: message i = base[i*stride ..
 * i*stride+len), any stride as for lsmck_crc32_batch_fixed: with stride < len
 * the messages overlap (host batches ship the span once). */
int lsmck_sha256_batch(lsmck_ctx* ctx, const uint8_t* base, const uint64_t* off, const uint32_t* len, size_t n,
                       uint8_t* out32, unsigned flags, void* stream);
int lsmck_sha256_batch_fixed(lsmck_ctx* ctx, const uint8_t* base, size_t stride, uint32_t len, size_t n,
                             uint8_t* out32, unsigned flags, void* stream);

/* WAL replay verify: the batch form of the CommandLog iterator + MemTable::from_log
 * (src/wal.rs:68-84,122-163; src/memtable.rs:28-47) over an in-memory WAL image.
 * Each record's length lives in its own header, so the walk is a dependent
 * chain.  On the GPU (lsmck_wal.hip) it is a speculative parallel parse: the
 * segment walk (lsmck_segwalk.h: one thread per segment of the log guesses
 * the segment's first record and walks the headers to the next segment; the
 * guesses are checked against each other and wrong ones repaired), or, when
 * its check keeps failing, candidate doubling (every byte that could start a
 * header is a candidate, candidate -> successor links followed by pointer
 * doubling from offset 0); the accepted chain's payload CRCs are checked in
 * one batch with the GPU compare.  A device image
 * never leaves the device; a host image of at least "wal_upload_min" bytes
 * (default 1 MiB) is uploaded whole and walked there; smaller host images
 * (and "wal_upload_min" 0) take the serial host walk with the CRC batches on
 * the GPU.  Results are the same on every path.
 * recs (optional, cap entries) receives the parsed records in log order.
 * Returns
 *   0                      clean end of log (header EOF ends iteration, wal.rs:76-77)
 *   LSMCK_WAL_CORRUPTED    first bad record is an Insert: WalError::CorruptedData
 *                          {checksum=*bad_crc, expected=*bad_expected} (wal.rs:136-141)
 *   LSMCK_WAL_REMOVE_PANIC first bad record is a Remove: the reference panics (wal.rs:154-159)
 *   LSMCK_WAL_BAD_TYPE     InvalidCommandType(*bad_crc) at record *bad_index (wal.rs:36)
 * *nrec = records accepted before the stop.  flags: LSMCK_HOST (optionally
 * | LSMCK_HOST_PINNED) or LSMCK_DEVICE for `wal`, optionally
 * | LSMCK_RECS_PINNED: `recs` is page-locked (lsmck_host_alloc_pinned), and
 * the records are DMA'd into it straight from the device (no staging copy),
 * or | LSMCK_RECS_DEVICE: `recs` is device memory (cap entries) and the
 * records stay there -- for a device-resident log whose consumer runs on the
 * GPU; the segment walk writes them in place when all of them fit, and no
 * record crosses the host link (any path that walks on the host copies its
 * records up).  In either array, entries past *nrec up to the walked record
 * count (records after a failed CRC) may be written too.  Synchronous. */
#define LSMCK_RECS_PINNED 0x8u
#define LSMCK_RECS_DEVICE 0x10u
#define LSMCK_WAL_CORRUPTED 1
#define LSMCK_WAL_REMOVE_PANIC 2
#define LSMCK_WAL_BAD_TYPE 3
typedef struct {
  uint64_t rec_off;     /* header offset */
  uint64_t payload_off; /* key offset */
  uint32_t klen, vlen;  /* vlen = 0 for Remove */
  uint32_t crc;         /* stored checksum */
  uint32_t type;        /* 1 Insert, 2 Remove */
} lsmck_wal_rec;
int lsmck_wal_replay_verify(lsmck_ctx* ctx, const uint8_t* wal, size_t n, unsigned flags, lsmck_wal_rec* recs,
                            size_t cap, size_t* nrec, uint64_t* bad_index, uint32_t* bad_crc,
                            uint32_t* bad_expected);

/* The same replay with compact records: 16 bytes each instead of 32 -- what
 * MemTable::from_log takes from a record (src/memtable.rs:28-47: the key and
 * value bytes and the command type).  The header offset is payload_off less
 * the header (13 bytes for Insert, 9 for Remove), and the stored CRC is not
 * kept: every accepted record's stored CRC equals its payload's CRC (a bad
 * one's comes back in *bad_expected).  Half the bytes cross the link when
 * the records go to the host (LSMCK_RECS_PINNED or a pageable array); with
 * LSMCK_RECS_DEVICE `recs` is a device array of lsmck_wal_rec16.  Flags,
 * returns and the other outputs as lsmck_wal_replay_verify.  Replaces the
 * same reference items. */
typedef struct {
  uint64_t payload_type; /* bits 0..62: payload (key) offset; bit 63: set for Remove, clear for Insert */
  uint32_t klen, vlen;   /* vlen = 0 for Remove */
} lsmck_wal_rec16;
#define LSMCK_WAL_REC16_REMOVE 0x8000000000000000ull
#define LSMCK_WAL_REC16_OFF_MASK 0x7FFFFFFFFFFFFFFFull
int lsmck_wal_replay_verify16(lsmck_ctx* ctx, const uint8_t* wal, size_t n, unsigned flags, lsmck_wal_rec16* recs,
                              size_t cap, size_t* nrec, uint64_t* bad_index, uint32_t* bad_crc,
                              uint32_t* bad_expected);

/* Batch framing of Insert records in a device-resident log, in place: payload
 * i (key || value, len[i] bytes) already lies at img + off[i], and its
 * 13-byte header (CommandLog::log, src/wal.rs:165-196) is written to
 * img + off[i] - 13 -- type 1, crc[i], klen = min(len[i], kmax), vlen = the
 * rest.  The batch form of lsmck_wal_encode_insert for logs built on the
 * GPU (a log of many GiB is framed in one launch); crc[i] is normally
 * lsmck_crc32_batch's output for the same payloads.  img, off, len, crc:
 * device pointers; asynchronous on `stream` (NULL = the context's stream).
 * Returns 0 or a negative hipError_t. */
int lsmck_wal_frame_insert_device(lsmck_ctx* ctx, uint8_t* img, const uint64_t* off, const uint32_t* len,
                                  const uint32_t* crc, size_t n, uint32_t kmax, void* stream);

/* Batch WAL encode: the batch form of CommandLog::log (src/wal.rs:165-196)
 * for a group commit, a memtable dump or a log built by a GPU-side producer --
 * the bulk append of the WAL seam, and the inverse of the replay's record
 * array.  Command i names its key in the `keys` arena and, for an Insert, its
 * value in the `vals` arena; img[0 .. *img_bytes) becomes byte for byte what
 * lsmck_wal_encode_insert / lsmck_wal_encode_remove give for commands 0..n-1
 * in order, concatenated -- the reference appending them one by one to an
 * empty log.  keys and vals may be the same buffer, and commands may name
 * overlapping or repeated source ranges; img must not overlap either arena.
 * On the device (lsmck_wal.hip): the record sizes are checked and scanned
 * into the record offsets; one gather kernel moves keys, values and header
 * fields into log order (the image cut into aligned tiles, every 16 aligned
 * bytes of it written by one 16-byte store); the payload CRCs come from the
 * dispatcher of lsmck_crc32_batch over the image (a log's payloads are sorted
 * and a header apart: the stream kernel); one thread per record stamps its CRC.
 * flags: LSMCK_DEVICE -- keys, vals, cmds (8-byte aligned), img and rec_off
 * are device pointers; LSMCK_HOST (optionally | LSMCK_HOST_PINNED) -- all of
 * them are host pointers: the arenas and the commands are uploaded whole, the
 * log is encoded on the device and the image copied back.  The host form is
 * staged whole, not pipelined, and its size is bounded by device memory
 * (arenas + commands + image).  LSMCK_HOST_PINNED is only a hint here: it
 * selects no other path -- every host buffer goes through hipMemcpyAsync on
 * the context's stream, which copies straight from and to the pages that are
 * pinned and stages the others -- so the buffers may be pinned one by one or
 * not at all.  Any other flag bit is LSMCK_EINVAL.  img_bytes and bad_index are host pointers
 * either way.  rec_off (optional, n entries) receives record i's header
 * offset.  Synchronous: the 8-byte total and the validation word are read
 * back after the offset scan, before anything is written to img.  Scratch
 * comes from the context; calls on one context serialise on it.
 * Returns 0 (n == 0: 0 and *img_bytes = 0), or
 *   LSMCK_EINVAL  a command's type is not 1 or 2; an Insert has klen + vlen >
 *                 2^32-1 (the reference's reader could not read it back:
 *                 data_len wraps at wal.rs:129, and the CRC batch takes u32
 *                 lengths); a non-empty key, or a non-empty value of an
 *                 Insert, reaches outside [0, keys_bytes) / [0, vals_bytes).
 *                 *bad_index = the first such command in batch order.  A
 *                 Remove's val_off and vlen are not looked at.
 *   LSMCK_ENOSPC  cap is smaller than the encoded size; *img_bytes = the
 *                 size needed.
 * On either error no byte of img is written. */
typedef struct {
  uint64_t key_off;    /* key   = keys[key_off .. key_off + klen) */
  uint64_t val_off;    /* value = vals[val_off .. val_off + vlen); ignored for Remove */
  uint32_t klen, vlen; /* vlen ignored (taken as 0) for Remove */
  uint32_t type;       /* 1 Insert, 2 Remove */
  uint32_t reserved;   /* 0 */
} lsmck_wal_cmd;       /* 32 bytes */
int lsmck_wal_encode_batch(lsmck_ctx* ctx, const uint8_t* keys, size_t keys_bytes, const uint8_t* vals,
                           size_t vals_bytes, const lsmck_wal_cmd* cmds, size_t n, uint8_t* img, size_t cap,
                           size_t* img_bytes, uint64_t* rec_off, uint64_t* bad_index, unsigned flags);

/* Host helper, no GPU: the bytes a batch encodes to (the sum of 13 + klen +
 * vlen per Insert and 9 + klen per Remove), or UINT64_MAX when a command is
 * invalid by itself (its type, or klen + vlen > 2^32-1 for an Insert). */
uint64_t lsmck_wal_encoded_size(const lsmck_wal_cmd* cmds, size_t n);

/* Batch SSTable encode: the batch form of SsTable::from_memtable's file
 * writes (src/tokio/sstable.rs:84-129, src/sync/sstable.rs:135-141,241-253)
 * and of merge_compact's (tokio/sstable.rs:135-192) for a bulk load, a flush
 * of many memtables or a compaction's output -- the write-side counterpart of
 * lsmck_checksums_verify_many: many tables encoded and hashed in one call.
 * Entries reuse lsmck_wal_cmd (type must be 1; a tombstone in the reference
 * is an ordinary pair whose value is [0]): entry i names its key in the
 * `keys` arena and its value in the `vals` arena; the arenas may be one
 * buffer, and source ranges may overlap or repeat.  Table t is entries
 * [table_first[t], table_first[t+1]) in that order; table_first (always a
 * HOST pointer, ntab + 1 values) starts at 0, ends at n and does not
 * decrease.  An empty table is allowed.
 *   data file of table t  = [u32 klen LE][u32 vlen LE][key][val] over its
 *     entries (datafile.rs:27-35); the tables' data files lie back to back
 *     in `data`, in table order, without padding;
 *   index file of table t = the bincode 1.x fixint image of the reference's
 *     BTreeMap<Vec<u8>, u64> (sstable_index.rs:42-46): u64 count =
 *     ceil(m_t / 100), then for every entry i of the table with i % 100 == 0
 *     u64 klen, the key, u64 pos -- the record's offset in its own table's
 *     data file; the index files lie back to back in `index` (an empty
 *     table's is the 8 bytes of a zero count);
 *   spans[t] (optional) = where table t's two files lie;
 *   data_sha[32t ..], index_sha[32t ..] = the SHA-256 of table t's data and
 *     index file (checksums.rs:64-80; the base64 and the JSON stay on the
 *     host: lsmck_base64_encode).  Either may be NULL: that image is not
 *     hashed.  One table is one sequential SHA-256 on one GPU lane.
 * flags: LSMCK_DEVICE -- keys, vals, ents (8-byte aligned), data, index,
 * spans and the digest arrays are device pointers; LSMCK_HOST (optionally
 * | LSMCK_HOST_PINNED, a hint only) -- all host pointers, staged whole as
 * lsmck_wal_encode_batch's host form is, bounded by device memory.  Any other
 * flag bit is LSMCK_EINVAL.  table_first, data_bytes, index_bytes and
 * bad_index are host pointers either way.  Synchronous; scratch comes from
 * the context, so calls on one context serialise.  The sizes and the error
 * words are read back once, before anything is written.
 * Returns 0 (n == 0 and ntab == 0: both sizes 0; n == 0 with ntab > 0: ntab
 * empty tables), or
 *   LSMCK_EINVAL  with *bad_index = the first offending entry in batch order:
 *                 its type is not 1; 8 + klen + vlen > 2^32-1 (the reference
 *                 forms the record size in u32, datafile.rs:34); a non-empty
 *                 source range lies outside its arena; or the entry is not
 *                 the first of its table and its key is not strictly greater
 *                 -- bytewise, a proper prefix first -- than its
 *                 predecessor's (the reference's memtable is a BTreeMap;
 *                 order across a table boundary is not checked).
 *                 With *bad_index = UINT64_MAX: table_first is malformed
 *                 (checked before any GPU work), n or ntab is 2^32 or more,
 *                 or a digest is asked for a table whose image is above
 *                 2^32-1 bytes (lsmck_last_error names the table).
 *   LSMCK_ENOSPC  data_cap or index_cap is too small; *data_bytes and
 *                 *index_bytes = the sizes needed.
 * On any error no byte of data, index, spans or the digest arrays is written. */
typedef struct {
  uint64_t data_off, data_len;   /* table t's data file  = data [data_off  .. data_off  + data_len)  */
  uint64_t index_off, index_len; /* table t's index file = index[index_off .. index_off + index_len) */
} lsmck_sstable_span;            /* 32 bytes */
int lsmck_sstable_encode_batch(lsmck_ctx* ctx, const uint8_t* keys, size_t keys_bytes, const uint8_t* vals,
                               size_t vals_bytes, const lsmck_wal_cmd* ents, size_t n, const uint64_t* table_first,
                               size_t ntab, uint8_t* data, size_t data_cap, uint8_t* index, size_t index_cap,
                               lsmck_sstable_span* spans, uint8_t* data_sha, uint8_t* index_sha, size_t* data_bytes,
                               size_t* index_bytes, uint64_t* bad_index, unsigned flags);

/* Host helper, no GPU: the two arena sizes a batch encodes to.  Returns 0, or
 * LSMCK_EINVAL when an entry is invalid by itself (its type, or 8 + klen +
 * vlen > 2^32-1) or table_first is malformed. */
int lsmck_sstable_encoded_size(const lsmck_wal_cmd* ents, size_t n, const uint64_t* table_first, size_t ntab,
                               uint64_t* data_bytes, uint64_t* index_bytes);

/* Batch memtable build: the batch form of MemTable::from_log's map
 * (src/memtable.rs:28-47) -- the step between the replay's records and
 * lsmck_sstable_encode_batch's sorted entries, for a log replayed on the GPU,
 * a group commit, several memtables flushed together or a bulk load.
 * Commands 0..n-1 are in log order (type 1 Insert, 2 Remove; arenas and ranges
 * as in lsmck_wal_encode_batch; a Remove's val_off and vlen are not looked at;
 * keys and vals may be one buffer).  ents[0 .. *nent) receives the live
 * entries as lsmck_wal_cmd of type 1, reserved 0, their ranges still pointing
 * into the caller's arenas, strictly increasing in the reference's
 * BTreeMap<Vec<u8>, _> order (bytewise, unsigned, a proper prefix first): per
 * distinct key the LAST command in log order when that is an Insert, nothing
 * when it is a Remove.  The array can be handed to lsmck_sstable_encode_batch
 * as it is.  src (optional): src[j] = the index in cmds of the command ents[j]
 * came from.  *mem_bytes = the reference's size_in_bytes() after from_log,
 * its quirk included: from_log adds klen + vlen for every Insert, also one
 * that overwrites (memtable.rs:37-38), and takes klen + vlen(current value)
 * away for a Remove that finds its key.
 * On the device (lsmck_memtable.hip, lsmck_memsort.h): the commands are
 * validated; the order is refined 8 key bytes a round -- the elements still
 * undecided sorted stably by (group, key bytes [8r, 8r+8) big-endian and zero
 * padded, min(klen - 8r, 9)) with a radix sort of fixed-width words, runs of
 * equal triples becoming the next round's groups, until no run of two or more
 * unfinished keys is left; the last element of each run of equal keys is the
 * key's last writer.  A pair of keys is separated in round lcp / 8, n copies
 * of a key of l bytes take about l / 8 rounds, and every round costs a host
 * round trip of 8 bytes (stat "mem_rounds"): keys of tens of bytes need 2-4
 * rounds, many copies of a key of several KiB need hundreds.
 * flags: LSMCK_DEVICE -- keys, vals, cmds (8-byte aligned), ents and src are
 * device pointers; LSMCK_HOST (optionally | LSMCK_HOST_PINNED, a hint only) --
 * host pointers, staged whole as lsmck_wal_encode_batch's host form is.  Any
 * other flag bit is LSMCK_EINVAL.  nent, mem_bytes and bad_index are host
 * pointers either way (nent and mem_bytes must not be NULL).  ents must not
 * overlap cmds.  Synchronous; scratch comes from the context, so calls on one
 * context serialise.  n >= 2^32 is LSMCK_EINVAL.
 * Returns 0 (n == 0: no entries, 0 bytes), or
 *   LSMCK_EINVAL  with *bad_index = the first offending command in batch
 *                 order: a type other than 1 or 2, or a non-empty key, or a
 *                 non-empty value of an Insert, outside its arena.
 *   LSMCK_ENOSPC  cap < *nent: *nent is the count needed, *mem_bytes is set.
 *   LSMCK_ENODEV  there is no GPU (and so no context).
 * On any error no byte of ents or src is written. */
int lsmck_memtable_build(lsmck_ctx* ctx, const uint8_t* keys, size_t keys_bytes, const uint8_t* vals,
                         size_t vals_bytes, const lsmck_wal_cmd* cmds, size_t n, lsmck_wal_cmd* ents, size_t cap,
                         uint32_t* src, size_t* nent, uint64_t* mem_bytes, uint64_t* bad_index, unsigned flags);

/* The replay's compact records (lsmck_wal_replay_verify16 with
 * LSMCK_RECS_DEVICE) as commands for lsmck_memtable_build, whose arenas are
 * the log image itself (keys == vals == the image, img_bytes long): key_off =
 * the payload offset, val_off = key_off + klen, type from bit 63, reserved 0.
 * The payload the reference read is short at the end of the log
 * (take().read_to_end, wal.rs:129-132): an Insert whose key lies wholly inside
 * the image has vlen cut to what the image holds, a Remove its klen.  An
 * Insert whose key is longer than the payload read (a key cut at the end of
 * the log, or a u32 wrap of klen + vlen) keeps a key that reaches past
 * img_bytes, so that the build reports LSMCK_EINVAL at that index: where the
 * reference's split_off panics (wal.rs:142).  recs and cmds are device
 * pointers; asynchronous on `stream` (NULL = the context's stream).  Returns
 * 0, a negative hipError_t code, or LSMCK_ENODEV without a GPU. */
int lsmck_wal_recs_to_cmds(lsmck_ctx* ctx, const lsmck_wal_rec16* recs, size_t n, uint64_t img_bytes,
                           lsmck_wal_cmd* cmds, void* stream);

/* Batch SSTable decode: the batch form of the data file's iterator
 * (src/sync/sstable.rs:77-90 over datafile.rs:60-83) -- the inverse of
 * lsmck_sstable_encode_batch, and the first step of a compaction on the
 * device (decode, lsmck_sstable_merge_batch, lsmck_sstable_encode_batch).
 * Table t's data file is data[spans[t].data_off .. + data_len) (the encode's
 * own span type; the tables may lie anywhere in the arena).  Its entries are
 * exactly the records the reference's iterator yields: from pos = 0, u32 klen
 * LE, u32 vlen LE, the key, the value; UnexpectedEof anywhere (a header cut
 * after 0..7 bytes, a key cut, a value cut) ends the table cleanly and the
 * partial record is dropped; pos advances by 8 + klen + vlen.  They are
 * written to ents[0 .. *nent), table after table, as lsmck_wal_cmd of type 1,
 * reserved 0, key_off and val_off pointing into `data`: the caller later
 * passes keys = vals = data.  tab_first (always a HOST pointer, ntab + 1
 * values) receives the tables' first entry numbers -- the table_first of the
 * merge and of the encode.  consumed (optional, ntab values) receives the
 * bytes each table's iterator got through, so that a caller can see a cut
 * tail (consumed[t] < data_len).  decode(encode(x)) == x entry for entry.
 * `index` (may be NULL) holds the tables' index files at spans[t].index_off /
 * index_len.  The chain of headers is serial inside a table: without an index
 * one GPU lane walks a table.  With one, the index -- the position of every
 * 100th record (sstable_index.rs:42-46) -- is a hint that is proven before it
 * is used: a thread per 100 records walks the headers from an item's position
 * and must land on the next item's.  The hint is taken for a table only if its
 * image parses to exactly index_len, pos_0 == 0, the positions increase inside
 * data_len, every segment passes exactly 100 records and lands on the next
 * position (an index whose keys have one length is parsed by a thread per
 * item: an item found in its expected place with that length proves the next
 * one's place), the last one ends after 1..100 records where the next record no
 * longer fits (an empty table: a count of 0 and no whole record).  Any other
 * table is walked by one lane (stat "sst_decode_declined" counts them).  The
 * entries never depend on the index: merge_compact does not read it.
 * flags: LSMCK_DEVICE -- data, index, spans, ents and consumed are device
 * pointers; LSMCK_HOST (optionally | LSMCK_HOST_PINNED, a hint only) -- host
 * pointers, staged whole.  Any other flag bit is LSMCK_EINVAL.  tab_first,
 * nent and bad_index are host pointers either way.  Synchronous; the total
 * and the error word are read back once, before anything is written.
 * Returns 0, or
 *   LSMCK_EINVAL  with *bad_index = the first table whose data span (or, with
 *                 an index, index span) lies outside its arena, or whose
 *                 data_len is above 2^32-1 (under that limit a record that
 *                 fits cannot wrap the reference's u32 8 + klen + vlen,
 *                 datafile.rs:81); with *bad_index = UINT64_MAX: an argument.
 *   LSMCK_ENOSPC  cap < *nent: *nent is the count needed.
 *   LSMCK_ENODEV  there is no GPU (and so no context).
 * On any error no byte of ents, tab_first or consumed is written. */
int lsmck_sstable_decode_batch(lsmck_ctx* ctx, const uint8_t* data, size_t data_bytes, const uint8_t* index,
                               size_t index_bytes, const lsmck_sstable_span* spans, size_t ntab, lsmck_wal_cmd* ents,
                               size_t cap, uint64_t* tab_first, uint64_t* consumed, size_t* nent, uint64_t* bad_index,
                               unsigned flags);

/* Host helper, no GPU, scalar: the records the reference's iterator yields
 * from the data file image img[0 .. n) (the walk above on the calling
 * thread); *consumed (optional) = the bytes it got through.  For callers that
 * size buffers.  Sizes are formed in 64 bits. */
uint64_t lsmck_sstable_count_records(const uint8_t* img, size_t n, uint64_t* consumed);

/* Batch compaction merge: the batch form of SsTable::merge_compact's loop
 * (src/sync/sstable.rs:151-224, src/tokio/sstable.rs:135-207; driven by
 * compact, sync/lsm_storage.rs:141-157) over sorted runs of entries -- the
 * decode's output, or any strictly increasing run: a memtable build's output
 * is a valid table.  Entries, arenas and tab_first as in
 * lsmck_sstable_encode_batch (tab_first: HOST, ntab + 1 entry numbers).
 * Group g merges tables [group_first[g], group_first[g + 1]) (group_first:
 * HOST, ngrp + 1 table numbers), oldest first, as in the reference's vector:
 * the loop scans the tables in vector order, `<=` moves the choice to the
 * later table on equal keys and the earlier table's equal entry is advanced
 * past (:171-189), so every distinct key comes out once, in Vec<u8> order
 * (bytewise, unsigned, a proper prefix first), taken from the
 * highest-numbered table of the group that holds it.  out[0 .. *nout)
 * receives the winners in key order, group after group, their ranges still
 * pointing into the caller's arenas; src (optional) the winner's index in
 * ents; out_first (HOST, ngrp + 1) the groups' first output entries -- the
 * table_first for lsmck_sstable_encode_batch.  Empty tables and empty groups
 * are allowed.
 * Tombstones (a winner whose value is the one byte 0): the reference's loop
 * does `continue` without advancing anything (:193-195) and never terminates.
 * By default the call returns LSMCK_MERGE_STUCK with *bad_index = the first
 * such winner in (group, key) order -- where the reference stops making
 * progress -- and writes nothing.  With LSMCK_MERGE_DROP_TOMBSTONES the key
 * leaves the output (what the reference's line plainly means to do); with
 * LSMCK_MERGE_KEEP_TOMBSTONES it stays as an ordinary pair (a merge above the
 * bottom level needs that to keep shadowing lower levels).  Both flags
 * together are LSMCK_EINVAL.  A tombstone that a newer table shadows is
 * harmless in every mode.
 * On the device (lsmck_sstmerge.hip, lsmck_sstmerge.h) the runs are not
 * sorted again: an entry is shadowed when a lower bound finds its key in a
 * newer table of its group; the live flags are scanned; a live entry's slot
 * is its group's base plus, over the group's tables, the live prefix at the
 * lower bound of its key.
 * flags: LSMCK_DEVICE -- keys, vals, ents (8-byte aligned), out and src are
 * device pointers; LSMCK_HOST (optionally | LSMCK_HOST_PINNED, a hint only)
 * -- host pointers, staged whole.  Synchronous; the count and the error
 * words are read back once, before anything is written.
 * Returns 0, LSMCK_MERGE_STUCK, or
 *   LSMCK_EINVAL  with *bad_index = the first offending entry: it fails
 *                 lsmck_sstable_encode_batch's entry rule (type, record size,
 *                 source ranges), or it is not the first of its table and
 *                 its key is not strictly greater than its predecessor's.
 *                 With *bad_index = UINT64_MAX (checked before any GPU
 *                 work): tab_first or group_first is malformed, n, ntab or
 *                 ngrp is 2^32 or more, an unknown flag or both tombstone
 *                 flags.
 *   LSMCK_ENOSPC  cap < *nout: *nout is the count needed.
 *   LSMCK_ENODEV  there is no GPU (and so no context).
 * On any error no byte of out, src or out_first is written. */
#define LSMCK_MERGE_STUCK 7
#define LSMCK_MERGE_DROP_TOMBSTONES 0x100u
#define LSMCK_MERGE_KEEP_TOMBSTONES 0x200u
int lsmck_sstable_merge_batch(lsmck_ctx* ctx, const uint8_t* keys, size_t keys_bytes, const uint8_t* vals,
                              size_t vals_bytes, const lsmck_wal_cmd* ents, size_t n, const uint64_t* tab_first,
                              size_t ntab, const uint64_t* group_first, size_t ngrp, lsmck_wal_cmd* out, size_t cap,
                              uint32_t* src, uint64_t* out_first, size_t* nout, uint64_t* bad_index, unsigned flags);

/* Batch point reads: the batch form of SsTable::get (src/sync/sstable.rs:97-113,
 * src/tokio/sstable.rs:57-82) over the tables of Db::get_internal's loop
 * (src/tokio/db.rs:178-185), for tables that stay device-resident (written by
 * lsmck_sstable_encode_batch, or uploaded).  Table t's data and index files lie
 * at spans[t] in `data` and `index` (the encode's span type).  Query i's key is
 * qkeys[q[i].key_off .. + klen); an empty key's offset is not looked at.
 * One key in one table, literally, quirks included:
 *   - The index file is the bincode fixint image of BTreeMap<Vec<u8>, u64>
 *     (sstable_index.rs:20-25).  It is taken as the map when it parses to
 *     exactly index_len bytes and its keys strictly increase in Vec<u8> order
 *     (bytewise, unsigned, a proper prefix first): file order is then map
 *     order and no key repeats.  ANY OTHER INDEX IS REFUSED -- the one
 *     deliberate refusal: the reference panics at load ("Can't open index
 *     file") or never writes such a file.  Positions may be any u64.
 *   - The map holds the key (sstable.rs:102-106): the result is the value of
 *     the record at the item's position WHATEVER ITS KEY IS -- the reference
 *     does not compare.  A position where no whole record fits gives None.
 *   - Otherwise position_range (sstable_index.rs:34-40): start = the position
 *     of the last item below the key, or 0; end = the position of the first
 *     item above it, or data_len.  scan_range (datafile.rs:85-103) reads the
 *     record at start EVEN WHEN start >= end, returns it when its key equals
 *     the key, else advances and stops once pos >= end or no whole record
 *     fits.  The scan is not bounded by 100 records: an index with an item
 *     missing makes an interval of 200.
 *   - read_record (datafile.rs:60-83): fewer than 8 bytes left, or a cut key
 *     or value, gives None.  data_len <= 2^32-1, as for the decode.
 *   - The bloom filter (sstable.rs:98) is not read: a filter built from the
 *     table's own keys has no false negatives, so it never changes a result,
 *     only the work.  The bloom file is out of scope, as everywhere here.
 * Over tables 0..ntab-1 IN THE ORDER GIVEN (search order: the caller passes
 * level 0 newest first, then level 1, and so on, as db.rs:178-185 iterates) a
 * key's result comes from the first table whose get is Some.  That includes a
 * tombstone, the one byte 0: get_internal stops there and Db::get turns it
 * into "not found" (db.rs:146-151).  res[i] says which of the three it is:
 *   table == LSMCK_GET_NONE           no table answered (val_off = 0, vlen = 0);
 *   val_off & LSMCK_GET_TOMBSTONE     table `table` answered with a tombstone
 *                                     (vlen = 1);
 *   otherwise                         the value is data[val_off .. + vlen).
 * Bits 0..62 of val_off hold the value's offset in `data` in every Some.
 * On the device (lsmck_sstget.hip, lsmck_sstget.h): an index pass leaves one
 * 16-byte order key, the offset and the position per index item (a thread per
 * item for an index of one key length, one lane per table otherwise) and
 * proves the key order; a work item per (query, table) pair does a lower bound
 * over the order keys and the exact hit's read or the interval's walk of
 * headers, and lowers the query's winning table with an atomic minimum; a
 * thread per query repeats the lookup in the winning table and writes res.
 * Db::get's memtable and old-memtable step in front of these tables, and the
 * values' bytes in one arena: lsmck_db_get_batch below.  A resident "opened
 * table" form that keeps the index pass between calls: lsmck_tableset_open
 * below.  Not covered: sorting queries by interval so that one walk serves
 * many.
 * flags: LSMCK_DEVICE -- data, index, spans, qkeys, q (8-byte aligned) and res
 * are device pointers; LSMCK_HOST (optionally | LSMCK_HOST_PINNED, a hint
 * only) -- host pointers, staged whole.  Any other flag bit is LSMCK_EINVAL.
 * bad_table and bad_query are host pointers (may be NULL) and are set to
 * UINT64_MAX unless they name something.  Synchronous; the error words are
 * read back once, before res is written.
 * Returns 0 (n == 0: nothing is written; ntab == 0: every result is
 * LSMCK_GET_NONE), or
 *   LSMCK_EINVAL  with *bad_table = the first table whose data or index span
 *                 lies outside its arena, whose data_len is above 2^32-1, or
 *                 whose index is refused under the rule above; else
 *                 with *bad_query = the first query whose non-empty key lies
 *                 outside [0, qkeys_bytes) or whose reserved != 0 (tables are
 *                 checked before queries); else
 *                 with both UINT64_MAX (checked before any GPU work): n or
 *                 ntab is 2^32 or more, index is NULL while ntab > 0, a null
 *                 array that is needed, or a wrong flag.
 *   LSMCK_ENODEV  there is no GPU (and so no context).
 * On any error no byte of res is written. */
typedef struct { uint64_t key_off; uint32_t klen; uint32_t reserved; } lsmck_get_query;   /* 16 bytes */
typedef struct { uint64_t val_off; uint32_t vlen; uint32_t table; } lsmck_get_result;     /* 16 bytes */
#define LSMCK_GET_NONE 0xFFFFFFFFu                 /* table: no table answered (val_off = 0, vlen = 0) */
#define LSMCK_GET_TOMBSTONE 0x8000000000000000ull  /* bit 63 of val_off: the value is the byte 0 */
int lsmck_sstable_get_batch(lsmck_ctx* ctx, const uint8_t* data, size_t data_bytes, const uint8_t* index,
                            size_t index_bytes, const lsmck_sstable_span* spans, size_t ntab, const uint8_t* qkeys,
                            size_t qkeys_bytes, const lsmck_get_query* q, size_t n, lsmck_get_result* res,
                            uint64_t* bad_table, uint64_t* bad_query, unsigned flags);

/* Host helper, no GPU, scalar: SsTable::get of one key in one table (the rules
 * above, the same code on the calling thread) -- the latency path.  Returns 1
 * (Some: *val_off = the value's offset in `data`, *vlen its length; a
 * tombstone is a Some of the one byte 0), 0 (None; both set to 0), or
 * LSMCK_EINVAL: the index is refused, data_len is above 2^32-1, or val_off or
 * vlen is NULL.  The index is parsed on every call (O(items)). */
int lsmck_sstable_get(const uint8_t* data, size_t data_len, const uint8_t* index, size_t index_len,
                      const uint8_t* key, uint32_t klen, uint64_t* val_off, uint32_t* vlen);

/* Batch Db::get: Db::get (src/tokio/db.rs:144-155) over Db::get_internal's
 * whole search order (db.rs:156-189, src/sync/lsm_storage.rs:101) for many
 * keys -- the memtable (db.rs:158-165), the old memtable (db.rs:166-173), then
 * the table loop (db.rs:178-185) -- with the values optionally gathered into
 * one packed arena.  A memtable is passed as a RUN: nent entries (the encode's
 * entry type, type 1) strictly increasing in Vec<u8> order, their key and
 * value ranges in the run's own two arenas (which may be one buffer) -- what
 * lsmck_memtable_build leaves.  Every run has its own arenas because a
 * memtable and an old memtable are separate buffers.
 *   Sources.  Sources 0..nrun-1 are the runs in the order given (the caller
 *     passes the memtable, then the old memtable); sources nrun..nrun+ntab-1
 *     are the tables in lsmck_sstable_get_batch's search order.  The first
 *     source whose get is Some answers.
 *   Runs.  A run's get is BTreeMap::get (memtable.rs:68-70): an entry whose
 *     key equals the query's key is Some(value).  An empty value counts, and
 *     so does the one byte 0: it is what Db::delete puts there (db.rs:140).
 *     A memtable rebuilt by from_log holds no tombstones -- its Removes erase
 *     entries (memtable.rs:40-43) -- so lsmck_memtable_build's output has
 *     none; a live memtable with deletes is built from Inserts of [0].
 *   Tables.  A table's get is lsmck_sstable_get_batch's, word for word: the
 *     same code, quirks included (see above).
 *   Results.  res[i].table is the source number or LSMCK_GET_NONE; val_off is
 *     relative to the winning run's `vals` (0 for an empty value: its offset
 *     is not looked at) or to `data`; the tombstone bit is set as above.  With
 *     nrun == 0 the results are byte-identical to lsmck_sstable_get_batch's.
 *   Gather (out_off != NULL).  out_off[0..n] is the exclusive scan of the
 *     answered lengths and out[out_off[i] .. out_off[i+1]) holds query i's
 *     value under Db::get's rule (db.rs:146-151): a tombstone winner or no
 *     winner contributes 0 bytes (res tells them apart from an empty value).
 *     A key asked twice is gathered twice.  *out_bytes = out_off[n].
 * On the device (lsmck_dbget.hip, lsmck_dbget.h): a thread per run entry
 * checks it, forms its 16-byte order key and proves it above its predecessor;
 * a work item per (query, run) pair does a lower bound over the order keys
 * (the arenas are read only on a tie past 8 bytes) before the table probe
 * starts, so a key a run answered walks no index interval; a thread per query
 * resolves its winner into scratch and the lengths are scanned there; the
 * error words and the total come back once; the gather is output-centric as
 * the encodes' are -- out cut into 32 KiB tiles aligned on its address, a lane
 * storing aligned 16-byte chunks once each, sources at any alignment.
 * flags: LSMCK_DEVICE -- every pointer inside the run descriptors, data, index,
 * spans, qkeys, q, res, out and out_off are device pointers (ents, q, res and
 * out_off 8-byte aligned); LSMCK_HOST (optionally | LSMCK_HOST_PINNED, a hint
 * only) -- host pointers, staged whole.  `runs` itself (nrun descriptors),
 * out_bytes and the bad_* words are host pointers either way; the bad_* words
 * may be NULL and are set to UINT64_MAX unless they name something.
 * Synchronous; scratch comes from the context.
 * Returns 0 (n == 0 with out_off: out_off[0] = 0), or, checked in this order,
 *   LSMCK_EINVAL  with *bad_run_entry = the first offending run entry, counted
 *                 across the runs: it fails the encode's entry rule (type 1,
 *                 8 + klen + vlen <= 2^32-1, non-empty ranges inside its own
 *                 run's arenas) or its key is not strictly above its
 *                 predecessor's in its run; else
 *                 with *bad_table, as lsmck_sstable_get_batch; else
 *                 with *bad_query, as lsmck_sstable_get_batch; or
 *                 with all three UINT64_MAX (checked before any GPU work): n,
 *                 ntab, nrun or the runs' entries together are 2^32 or more, a
 *                 null array that is needed, out_off without out_bytes, or a
 *                 wrong flag.
 *   LSMCK_ENOSPC  out_cap is smaller than the gathered bytes: *out_bytes is
 *                 the size needed.
 *   LSMCK_ENODEV  there is no GPU (and so no context).
 * On any error no byte of res, out_off or out is written. */
typedef struct {
  const uint8_t* keys; uint64_t keys_bytes;   /* the run's arenas (may be one buffer) */
  const uint8_t* vals; uint64_t vals_bytes;
  const lsmck_wal_cmd* ents; uint64_t nent;   /* type 1, strictly increasing in Vec<u8> order */
} lsmck_get_run;                              /* 48 bytes; the array itself is always a HOST array of nrun */
int lsmck_db_get_batch(lsmck_ctx* ctx, const lsmck_get_run* runs, size_t nrun, const uint8_t* data, size_t data_bytes,
                       const uint8_t* index, size_t index_bytes, const lsmck_sstable_span* spans, size_t ntab,
                       const uint8_t* qkeys, size_t qkeys_bytes, const lsmck_get_query* q, size_t n,
                       lsmck_get_result* res, uint8_t* out, size_t out_cap, uint64_t* out_off, uint64_t* out_bytes,
                       uint64_t* bad_run_entry, uint64_t* bad_table, uint64_t* bad_query, unsigned flags);

/* Opened table set: SsTable::load (src/tokio/sstable.rs:32-55) for many tables
 * once, then Db::get (src/tokio/db.rs:156-189) over them call after call -- a
 * reader loads its tables once and serves gets until a compaction replaces
 * them.  lsmck_tableset_open runs lsmck_sstable_get_batch's index pass once
 * and keeps what it proves (spans, per item the order key, offset and
 * position) in buffers the set owns, never in the context's scratch; and it
 * computes per table two KEY FENCES.  With items (key_j, pos_j), j < m, and
 * data length L (m == 0: no fence):
 *   low   the walk of scan_range(0, pos_0): the record at 0 is attempted even
 *         when pos_0 is 0, then the walk goes on while pos < pos_0 and a whole
 *         record fits.  Valid when it ends within "fence_walk_cap" records and
 *         no visited key is below key_0: then every k < key_0 is None.
 *   high  the walk of scan_range(pos_{m-1}, L) by the same rule.  Valid when it
 *         ends within the cap; hi = max(key_{m-1}, the visited keys): then
 *         every k > hi is None.
 * Both follow from the literal SsTable::get alone (lsmck_tableset.h has the
 * argument), for positions that are any u64, records that hold any key, and
 * tails that are unsorted or cut: a fenced (query, table) pair costs two key
 * compares and no lookup, and no result differs.
 * BLOOM FILTERS ("bloom_bits" > 0): the role of SsTable::get's first line
 * (src/sync/sstable.rs:98), built from the tables' own bytes at open and kept
 * on the device; not the reference's bloom file.  A table's key set is every
 * item key of at most 2^32-1 bytes and the key of every record its m + 1
 * interval walks visit (scan_range(0, pos_0), scan_range(pos_j, pos_{j+1}),
 * scan_range(pos_{m-1}, L); m == 0: scan_range(0, L)); the table has a filter
 * when each walk ends within "fence_walk_cap" records.  SsTable::get answers
 * Some only for an item key or for a record one of those walks visits, so a
 * pair the filter drops is None whatever the table's bytes are
 * (lsmck_bloom.h has the argument and the split-block layout); a table
 * without a filter is simply looked up.  A get hashes every query once and
 * tests a pair that passed the fences with one 32-byte load.
 * open (tokio/sstable.rs:32-55).  The rules, the refusals, the first
 * bad_table and the cases checked before any GPU work are
 * lsmck_sstable_get_batch's, word for word.  flags: LSMCK_DEVICE -- data,
 * index and spans are device pointers and the set BORROWS data and index: the
 * caller keeps them alive and unchanged until lsmck_tableset_close (item keys
 * that tie past 8 bytes still read index bytes; spans is copied); LSMCK_HOST
 * (optionally | LSMCK_HOST_PINNED) -- host pointers, and the set OWNS device
 * copies, staged once: the caller's arrays are free after return.  ntab == 0
 * is a valid set.  On any error *set = NULL and nothing is retained.  `set`
 * and bad_table (may be NULL) are host pointers.
 * get (tokio/db.rs:156-189).  lsmck_db_get_batch with the set in place of
 * (data, index, spans): meaning, result encoding (val_off relative to the
 * arena the set was opened over), gather, error order and "no byte written on
 * error" are that call's word for word, but that no table can be refused any
 * more.  `flags` describe the per-call pointers alone -- the run descriptors'
 * pointers, qkeys, q, res, out, out_off -- host or device whichever way the
 * set was opened.  A set used with a context other than the one that opened
 * it, or a NULL set, is LSMCK_EINVAL.  On the device (lsmck_tableset.hip): the
 * kernels of lsmck_db_get_batch without the index pass, and a table probe
 * that tests the fences before it looks anything up.
 * stat.  "tables", "items" (index items of all tables), "fenced_low" and
 * "fenced_high" (the tables with each fence), "bloom_tables" (the tables with
 * a filter), "bloom_keys" (their keys, duplicates counted), "bloom_bytes" (the
 * filters' blocks and the 16-byte descriptor per table; 0 for a set opened
 * without filters), "resident_bytes" (device bytes the set owns, the filters'
 * among them).  LSMCK_EINVAL for an unknown key or a NULL argument.
 * close.  Frees the set; NULL is a no-op.  Sets are closed before their
 * context is destroyed.
 * With "sst_encode_time" 1, lsmck_ctx_get_stat has "tableset_open_index_ns",
 * "tableset_open_fence_ns" and "tableset_open_bloom_ns" (the filters' count,
 * sizes and fill; 0 without them) for the last open, and for the last get
 * "tableset_runs_ns", "tableset_run_probe_ns", "tableset_probe_ns",
 * "tableset_resolve_ns", "tableset_gather_ns", and "tableset_probed" /
 * "tableset_walked" / "tableset_fenced": the (query, table) pairs looked up,
 * those whose interval was walked, and those the fences dropped (counted
 * before the check for a lower source's answer, so a fixed number per input);
 * and "tableset_bloomed": the pairs that passed the fences and that the
 * filters dropped, counted the same way.
 * Not covered: an opened run form, sorting queries by interval, a
 * host-resident opened table for the scalar lsmck_sstable_get, fences for a
 * table without index items, the reference's bloom file (bincode of a crate's
 * filter with hashers keyed from entropy), filters for runs. */
typedef struct lsmck_tableset lsmck_tableset;
int lsmck_tableset_open(lsmck_ctx* ctx, const uint8_t* data, size_t data_bytes, const uint8_t* index,
                        size_t index_bytes, const lsmck_sstable_span* spans, size_t ntab, lsmck_tableset** set,
                        uint64_t* bad_table, unsigned flags);
int lsmck_tableset_get_batch(lsmck_ctx* ctx, const lsmck_tableset* set, const lsmck_get_run* runs, size_t nrun,
                             const uint8_t* qkeys, size_t qkeys_bytes, const lsmck_get_query* q, size_t n,
                             lsmck_get_result* res, uint8_t* out, size_t out_cap, uint64_t* out_off,
                             uint64_t* out_bytes, uint64_t* bad_run_entry, uint64_t* bad_query, unsigned flags);
int lsmck_tableset_stat(const lsmck_tableset* set, const char* key, long* value);
void lsmck_tableset_close(lsmck_tableset* set);

/* Batch write plan: the batch form of the memtable side of LsmStorage::insert
 * and LsmStorage::delete (src/sync/lsm_storage.rs:59-78, 133-139) -- where a
 * command stream flushes, and what every flushed memtable holds.  Commands
 * 0..n-1 (type 1 Insert, 2 delete; arenas and ranges as in
 * lsmck_memtable_build, a delete's val_off and vlen are not looked at) are
 * applied in order to an empty memtable, each as MemTable::insert
 * (memtable.rs:72-79): an Insert puts (key, value), a delete puts (key, [0])
 * (lsm_storage.rs:137), and size_in_bytes() stays the sum of klen + vlen over
 * the pairs held -- an overwrite takes the pair it replaces away, unlike
 * from_log's count.  After an Insert, and only then, size_in_bytes() >= limit
 * flushes (lsm_storage.rs:65; >= as in the sync engine): the memtable ends
 * with this command and the next command starts an empty one.  A delete never
 * flushes, also when it takes the size past the limit; limit 0 flushes after
 * every Insert.
 * The result is *nflush closed segments and one open one, the memtable left
 * (empty when the last command flushed): segs[0 .. *nflush] -- *nflush + 1
 * items -- with segment g the commands [segs[g].first_cmd, segs[g+1].first_cmd)
 * (n closes the last) and the entries [segs[g].first_ent, segs[g+1].first_ent)
 * (*nent closes the last) of ents; segs[g].mem_bytes = size_in_bytes() at the
 * segment's end.  A segment's entries are the last writer of every distinct
 * key among its commands, in BTreeMap<Vec<u8>, _> order, as lsmck_wal_cmd of
 * type 1, reserved 0, their ranges in the caller's arenas; a delete's entry
 * has val_off = tomb_off and vlen = 1, and vals[tomb_off] must be a 0 byte the
 * caller placed there (looked at only when the batch holds a delete).  The
 * first_ent values of the closed segments are lsmck_sstable_encode_batch's
 * table_first and ents its entries, unchanged.  src (optional): src[j] = the
 * command ents[j] came from.
 * Not modelled: a replayed memtable in front of the stream, the tokio
 * engine's old_memtable, compact() behind a flush (lsm_storage.rs:74; it moves
 * no cut), the bloom file.  Reads between the writes are
 * lsmck_db_apply_plan's, below.
 * On the device (lsmck_writeplan.hip, lsmck_writeplan.h): the memtable
 * build's rounds order the commands by (key, log position); from that every
 * command's predecessor with the same key.  A thread per candidate start
 * walks its memtable for at most "cut_walk_cap" commands; the starts are cut
 * into blocks of "cut_block", per block the orbits' exits are found by
 * pointer doubling in LDS, one workgroup follows the true starts from block
 * to block and resolves a start whose walk met the cap by windows of its
 * width; a scan numbers the segments, a stable radix sort by segment number
 * keeps key order inside each.
 * flags: LSMCK_DEVICE -- keys, vals, cmds, ents, src and segs are device
 * pointers, 8-byte aligned; LSMCK_HOST (optionally | LSMCK_HOST_PINNED, a hint
 * only) -- host pointers, staged whole (the value arena is not: one byte of it
 * is).  Any other flag bit is LSMCK_EINVAL.  nent, nflush and bad_index are
 * host pointers either way (nent and nflush must not be NULL).  Synchronous;
 * scratch comes from the context.  n >= 2^32 is LSMCK_EINVAL.
 * Returns 0 (n == 0: one open segment {0, 0, 0}), or
 *   LSMCK_EINVAL  with *bad_index = the first offending command: one
 *                 lsmck_memtable_build refuses, or one whose entry would be
 *                 too long for a table (8 + klen + vlen > 2^32-1); with
 *                 *bad_index = UINT64_MAX: a delete is there and the
 *                 tombstone byte lies past the arena or is not 0.
 *   LSMCK_ENOSPC  ent_cap < *nent or seg_cap < *nflush + 1: both counts are
 *                 the ones needed.
 *   LSMCK_ENODEV  there is no GPU (and so no context).
 * On any error no byte of ents, src or segs is written. */
typedef struct { uint64_t first_cmd, first_ent, mem_bytes; } lsmck_write_seg;   /* 24 bytes */
int lsmck_db_write_plan(lsmck_ctx* ctx, const uint8_t* keys, size_t keys_bytes, const uint8_t* vals, size_t vals_bytes,
                        const lsmck_wal_cmd* cmds, size_t n, uint64_t limit, uint64_t tomb_off,
                        lsmck_wal_cmd* ents, size_t ent_cap, uint32_t* src,
                        lsmck_write_seg* segs, size_t seg_cap,
                        size_t* nent, size_t* nflush, uint64_t* bad_index, unsigned flags);

/* Host helper, no GPU: the same call on one thread with a std::map -- the
 * scalar fallback, host pointers only.  The same results and errors (no
 * LSMCK_ENODEV). */
int lsmck_db_write_plan_cpu(const uint8_t* keys, size_t keys_bytes, const uint8_t* vals, size_t vals_bytes,
                            const lsmck_wal_cmd* cmds, size_t n, uint64_t limit, uint64_t tomb_off,
                            lsmck_wal_cmd* ents, size_t ent_cap, uint32_t* src,
                            lsmck_write_seg* segs, size_t seg_cap,
                            size_t* nent, size_t* nflush, uint64_t* bad_index);

/* Batch command stream: lsmck_db_write_plan with Gets between the writes --
 * the commands of src/command.rs in arrival order, every get seeing every
 * write before it (LsmStorage::get, src/sync/lsm_storage.rs:99-125).  Commands
 * 0..n-1 have type 1 Insert (an update is an Insert, lsm_storage.rs:128),
 * 2 delete or LSMCK_CMD_GET; arenas and ranges as in lsmck_db_write_plan, a
 * Get's val_off and vlen are not looked at.  They are applied in order to an
 * LsmStorage whose memtable is empty, whose compact() is deferred and whose
 * tables -- "the base" -- are the caller's.
 * Writes.  lsmck_db_write_plan's rules, word for word.  A Get changes
 * nothing: it adds no bytes and never flushes; it counts as a command in
 * first_cmd (and towards "cut_walk_cap").  With every Get removed and the
 * indices renumbered, ents, *nent, *nflush, mem_bytes and first_ent are
 * lsmck_db_write_plan's output on the remaining commands, src and first_cmd
 * the same after renumbering; a stream without Gets yields byte-identical
 * outputs.  One new shape: the open segment may hold only Gets (a stream of
 * Gets, or Gets behind a final flush): first_cmd < n, no entries, first_ent =
 * *nent, mem_bytes = 0.
 * Gets.  The reference asks the memtable, then level 0 newest first, then the
 * lower levels; the stream's flushes are pushed behind the base's level-0
 * tables, so they are met first, newest first, and a table written by
 * from_memtable finds exactly the keys it holds.  So the Get at command i is
 * answered by the last write j < i with its key, if there is one: by the
 * memtable when j lies in i's segment (source = LSMCK_APPLY_MEMTABLE), else
 * by the table that j's segment g was flushed to (source = g).  The answer is
 * that write's value in vals: val_off / vlen of an Insert (val_off = 0 for an
 * empty value), tomb_off and 1 for a delete; a delete, or an Insert of the
 * single byte 0, carries LSMCK_GET_TOMBSTONE in bit 63 of val_off (Db::get's
 * rule, as in lsmck_get_result).  With no such write the Get is a miss: source
 * = LSMCK_GET_NONE, val_off = 0, vlen = 0, src_cmd = 0xFFFFFFFF, and the base
 * answers it.
 * gets[0 .. *nget) holds the Gets in stream order.  miss_q / miss_get
 * (optional: both or both NULL, get_cap items each) hold the misses in stream
 * order: {key_off, klen, 0} into keys, and the miss's index in gets -- queries
 * of lsmck_tableset_get_batch or lsmck_db_get_batch with qkeys = keys.  *nmiss
 * is reported also without them.
 * On the device (lsmck_apply.hip, lsmck_apply.h): the write plan's kernels but
 * four pieces that look at a key's run of the order, where Gets now stand
 * between the writes -- the validation; prev, a write's previous *write*,
 * which also answers a Get, from two max-scans over the order (the run's
 * start, the last write); the entry flags, every write clearing the previous
 * write of its (segment, key); and the Gets' and misses' slots from two scans
 * over the stream.
 * Flags, alignment (gets and miss_q 8-byte aligned, miss_get 4), synchrony,
 * scratch and the 2^32 limit: lsmck_db_write_plan's; the host form stages the
 * value arena whole.  nent, nflush, nget and nmiss must not be NULL.
 * Returns 0 (n == 0: one open segment {0, 0, 0}, all counts 0), or
 *   LSMCK_EINVAL  as lsmck_db_write_plan, in its order: the type check takes
 *                 1, 2 and 3, a Get's key range is checked like any key, the
 *                 entry-length and tombstone-byte rules hold for writes only.
 *   LSMCK_ENOSPC  ent_cap < *nent, seg_cap < *nflush + 1 or get_cap < *nget:
 *                 all four counts are the ones needed.
 *   LSMCK_ENODEV  there is no GPU (and so no context).
 * On any error no byte of any output array is written.
 * lsmck_ctx_get_stat: "cut_steps", "cut_long" and "mem_rounds" as for the
 * write plan, "apply_gets" and "apply_misses" for the last stream; with
 * "mem_build_time" 1 the last call's stages between device events:
 * "apply_order_ns" (validation and the rounds), "apply_prep_ns" (the packed
 * words, both scans, prev), "apply_walk_ns", "apply_chain_ns", "apply_mark_ns"
 * (the marks, the entry flags, the slots' scans) and "apply_emit_ns" (the
 * Gets, the entries, the segments).
 * Not modelled: a memtable that holds entries in front of the stream, the
 * tokio engine's old_memtable, compact() behind a flush (it can resurrect a
 * deleted key through the merge's tombstone drop), gathering the answers into
 * a packed arena, merging the base's answers into gets. */
#define LSMCK_CMD_GET 3u
#define LSMCK_APPLY_MEMTABLE 0xFFFFFFFEu
typedef struct {
  uint64_t val_off;  /* in vals; bit 63 LSMCK_GET_TOMBSTONE; 0 for an empty value and for a miss */
  uint32_t vlen;
  uint32_t source;   /* LSMCK_APPLY_MEMTABLE, the flushed table (segment number), or LSMCK_GET_NONE */
  uint32_t cmd;      /* the Get's index in cmds */
  uint32_t src_cmd;  /* the write that answers, 0xFFFFFFFF for a miss */
} lsmck_apply_get;   /* 24 bytes */
int lsmck_db_apply_plan(lsmck_ctx* ctx, const uint8_t* keys, size_t keys_bytes, const uint8_t* vals, size_t vals_bytes,
                        const lsmck_wal_cmd* cmds, size_t n, uint64_t limit, uint64_t tomb_off,
                        lsmck_wal_cmd* ents, size_t ent_cap, uint32_t* src,
                        lsmck_write_seg* segs, size_t seg_cap,
                        lsmck_apply_get* gets, size_t get_cap, lsmck_get_query* miss_q, uint32_t* miss_get,
                        size_t* nent, size_t* nflush, size_t* nget, size_t* nmiss, uint64_t* bad_index,
                        unsigned flags);

/* Host helper, no GPU: the same call on one thread with a std::map, host
 * pointers only.  The same results and errors (no LSMCK_ENODEV). */
int lsmck_db_apply_plan_cpu(const uint8_t* keys, size_t keys_bytes, const uint8_t* vals, size_t vals_bytes,
                            const lsmck_wal_cmd* cmds, size_t n, uint64_t limit, uint64_t tomb_off,
                            lsmck_wal_cmd* ents, size_t ent_cap, uint32_t* src,
                            lsmck_write_seg* segs, size_t seg_cap,
                            lsmck_apply_get* gets, size_t get_cap, lsmck_get_query* miss_q, uint32_t* miss_get,
                            size_t* nent, size_t* nflush, size_t* nget, size_t* nmiss, uint64_t* bad_index);

/* Whole-tree SSTable verify: the batch form of Checksums::verify over many
 * tables (Db::load, src/tokio/db.rs:37-59 -> src/tokio/sstable.rs:34).
 * Streams every data/index file in slices: 8192 files in flight (largest
 * first), 128 KiB of each per round, 16 reader threads filling one pinned slot
 * while the GPU hashes the previous round (per-file SHA-256 state carried on
 * the device), then compares with each checksum file.  Files of 16 MiB and
 * more are hashed on host threads meanwhile (one file is one sequential
 * SHA-256: a GPU lane would take ~1 s per 16 MB).  status[i] gets table i's
 * lsmck_checksums_verify status (0, the LSMCK_PANIC_OPEN_* codes,
 * LSMCK_DATA_MISMATCH / LSMCK_INDEX_MISMATCH, -errno, LSMCK_EJSON; -EAGAIN: a
 * file shrank while it was read).  Returns the number of tables whose status
 * is not 0. */
int lsmck_checksums_verify_many(lsmck_ctx* ctx, const char* const* data_paths, const char* const* index_paths,
                                const char* const* checksum_paths, size_t n, int* status);

/* Db::load's whole checksum scan of a tree (src/tokio/db.rs:37-59): for
 * level-0 .. level-4 under `base` (created if missing, fs::create_dir_all),
 * every directory entry whose UTF-8 name contains "metadata" is parsed as
 * SsTableMetadata JSON (sstable_metadata.rs:76-83) and the table it names --
 * base_path/level-<level>/{data,index,checksum}_filename -- is verified as by
 * lsmck_checksums_verify_many.  Metadata parsing runs on 8 host threads.  Returns 0 when every table verifies, 1 when some table
 * does not (rep->first_* names the first one in load order: level, then
 * read_dir order -- the table where the reference's loop panics or errors),
 * or a negative error (creating or listing a level directory failed).
 * first_status is a lsmck_checksums_verify_many status or LSMCK_META_PANIC:
 * the metadata file is unreadable or not valid SsTableMetadata JSON, where
 * the reference panics with "Can't open metadata file" / "Can't read metadata
 * file, file with unknown format" (sstable_metadata.rs:77-83). */
#define LSMCK_SSTABLE_MAX_LEVEL 5 /* src/tokio/db.rs:17 */
#define LSMCK_META_PANIC 3
typedef struct {
  uint64_t tables;      /* metadata entries found */
  uint64_t table_bytes; /* data + index bytes hashed */
  uint64_t bad_tables;  /* tables with a non-zero status */
  uint64_t first_index; /* load-order index of the first bad table (UINT64_MAX: none) */
  int first_status;
  int reserved;
  double list_seconds;   /* listing + metadata parsing */
  double verify_seconds; /* the lsmck_checksums_verify_many part, split as: */
  double stat_seconds;   /*   sizing the files */
  double read_seconds;   /*   reader threads filling the pinned slots */
  double gpu_wait_seconds; /* waiting for a slot's copy + kernels, final digest copy */
  double compare_seconds;  /*  reading the checksum files, comparing */
  uint64_t rounds;         /*  slice rounds */
  uint64_t fds_cached;     /*  files kept open between slices (RLIMIT_NOFILE bound) */
  char first_metadata_path[4096];
} lsmck_tree_report;
int lsmck_tree_verify(lsmck_ctx* ctx, const char* base, lsmck_tree_report* rep);

/* The same verify, handing the caller the listing it made: `fn` is called once,
 * after every metadata file is parsed and before the tables are hashed, with
 * the tables in load order (per level, read_dir order).  The entries live until
 * lsmck_tree_verify_listed returns, so the caller can load the tables' read
 * path (their sparse indexes) beside the verify instead of opening every
 * metadata file again -- Db::load's other half (src/tokio/db.rs:40-55 ->
 * SsTable::load).  fn may be NULL. */
typedef struct {
  const char* metadata_path;
  const char* data_path;     /* construct_path: base_path/level-<level>/data_filename (sstable_metadata.rs:43-48) */
  const char* index_path;
  const char* checksum_path;
  const char* id;            /* the metadata's u128 id, decimal */
  unsigned level;
  int status;                /* 0, or LSMCK_META_PANIC: not SsTableMetadata JSON (paths and id "") */
} lsmck_table_entry;
typedef void (*lsmck_tree_listed_fn)(void* user, const lsmck_table_entry* tables, size_t n);
int lsmck_tree_verify_listed(lsmck_ctx* ctx, const char* base, lsmck_tree_report* rep, lsmck_tree_listed_fn fn,
                             void* user);

/* The same over several devices of one node: the tables are split
 * into contiguous runs balanced by bytes, one per context (one host thread,
 * one set of pinned slots and one PCIe link each), verified concurrently; no
 * data moves between devices.  Statuses and the report are those of the
 * single-context call (timings: the slowest device's). */
int lsmck_tree_verify_multi(lsmck_ctx* const* ctxs, size_t nctx, const char* base, lsmck_tree_report* rep);
int lsmck_checksums_verify_many_multi(lsmck_ctx* const* ctxs, size_t nctx, const char* const* data_paths,
                                      const char* const* index_paths, const char* const* checksum_paths, size_t n,
                                      int* status);

/* ======================================================================== */
/* 4. Plumbing for hosts without their own HIP bindings (tests, bench)        */
/* ======================================================================== */
void* lsmck_dev_alloc(lsmck_ctx* ctx, size_t bytes);       /* hipMalloc */
void lsmck_dev_free(lsmck_ctx* ctx, void* p);
void* lsmck_host_alloc_pinned(lsmck_ctx* ctx, size_t bytes); /* hipHostMalloc */
void lsmck_host_free_pinned(lsmck_ctx* ctx, void* p);
int lsmck_memcpy_h2d(lsmck_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream);
int lsmck_memcpy_d2h(lsmck_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream);
int lsmck_memset_dev(lsmck_ctx* ctx, void* dst, int value, size_t bytes, void* stream);
int lsmck_stream_sync(lsmck_ctx* ctx, void* stream);
/* Synthetic records: device byte stream, byte b = byte (b%8) of
 * splitmix64(seed ^ (b/8)) for b in [byte_off, byte_off+n). */
int lsmck_gen_stream(lsmck_ctx* ctx, uint8_t* dst_dev, uint64_t seed, uint64_t byte_off, size_t n, void* stream);
/* Zipf(s) lengths on k=1..kmax, L = max(lmin, 64k - j), j ~ U{0..63} (host). */
void lsmck_gen_zipf_lengths(uint64_t seed, double s, int kmax, uint32_t lmin, size_t n, uint32_t* out);
/* records [first, first + n) of the same stream (record r's length depends on
 * (seed, r) alone): one rank's share of a global config-3 stream */
void lsmck_gen_zipf_lengths_at(uint64_t seed, double s, int kmax, uint32_t lmin, uint64_t first, size_t n,
                               uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* LSMCK_H */
