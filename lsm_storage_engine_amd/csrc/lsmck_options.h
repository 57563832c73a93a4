// lsmck_options.h -- lsmck_ctx_set_option's options as data: the values with
// their defaults (Options), and one table row per option with its name and the
// values it takes (kOptions).  What each option does is documented with
// lsmck_ctx_set_option in include/lsmck.h.  Host C++ only, nothing from HIP.
#ifndef LSMCK_OPTIONS_H
#define LSMCK_OPTIONS_H
#include <limits.h>
#include <string.h>

#include <string>

#include "lsmck.h"

namespace lsmck_host {

// Every field is a long (what lsmck_ctx_set_option takes); a reader that needs
// a narrower type casts where it reads -- the ranges below make that safe.
struct Options {
  long crc_ablate = 0, sha_order = 1, crc_stream = 1;  // kept as bits of `variant`, which the kernels' launchers take
  long variant = 0;                                    // (not an option itself: see kVariant*)
  // whole-tree verify (0: the built-in value)
  long tree_active_files = 0, tree_slice_bytes = 0, tree_list_batch = 0, tree_overlap = 2048, tree_json_threads = 0;
  long tree_stages = 3, tree_open_files = -1, tree_cpu_file_bytes = 0, tree_list_threads = 0, tree_readers = 16;
  // host staging
  long stage_threads = 8, stage_numa = -2;
  // WAL replay (wal_stage_bytes 16 MiB: 6.3 ms for the 0.24 GB wal_diag image against 6.5 at 64 MiB -- the first
  // copy and the last DMA are not overlapped -- and 10.7 at 4 MiB, per-chunk costs; profiles/r03/h/wal_diag_r03h.json)
  long wal_chunk_bytes = 32l << 20, wal_gpu_walk = 1, wal_stage_bytes = 16l << 20, wal_part_bytes = 0, wal_split = 1;
  long wal_register = 0, wal_upload_min = 1l << 20, wal_dma_engines = 4, wal_dma_chunks = 32, wal_prefetch = 4096;
  // ... its segment walk
  long wal_seg_walk = 1, wal_seg_bytes = 0, wal_seg_stage = 1, wal_seg_pack = 1, wal_seg_prepair = 2;
  long wal_seg_rounds = 16;
  // ... its pipelined form
  long wal_pipe = 0, wal_pipe_first = 4, wal_pipe_cus = 32, wal_pipe_min = 1l << 30, wal_pipe_seg = 0;
  long wal_pipe_layout = 0;
  // SHA-256 batches
  long sha_bucket_from = 128, sha_bucket_shift = 2, sha_short_blocks = 12, sha_pair = 1;
  // diagnostics: the batch builders' stages between device events
  long wal_encode_time = 0, sst_encode_time = 0, mem_build_time = 0;
  // the batch write plan: a candidate start's walk steps at most, the starts a workgroup links in LDS
  long cut_walk_cap = 4096, cut_block = 8192;
  // the opened table set: the records a fence's walk visits at most (lsmck_tableset.h; read when a set is opened)
  long fence_walk_cap = 256;
  // ... and the bits per key of its tables' resident bloom filters, 0: none (lsmck_bloom.h; read when a set is opened)
  long bloom_bits = 0;
};

// `variant` bits
constexpr long kVariantAblate = 0xF00;         // crc_ablate << 8
constexpr long kVariantBatchOrder = 0x10000;   // sha_order 0: variable-length SHA batches in batch order (A/B)
constexpr long kVariantNoStream = 0x200000;    // crc_stream 0: no stream kernel for descriptor batches (A/B)
constexpr long kVariantStreamOnly = 0x400000;  // crc_stream 2: the stream kernel alone (diagnostic)

// what the range of an option depends on besides the table
struct OptionEnv {
  int ncu;        // the device's compute units
  bool ab_build;  // the library was built with the A/B ablations
};

struct OptionRow {
  const char* name;
  long Options::*field;
  long lo, hi;            // accepted: lo..hi ...
  bool zero_too = false;  // ... and 0 (below lo)
  long multiple = 1;      // ... in multiples of this
  // not plain: the row's own check (null: the range above) and what follows the store
  bool (*accepts)(const OptionRow&, long, const OptionEnv&, std::string* why) = nullptr;
  void (*stored)(Options&) = nullptr;
};

inline std::string option_range(const OptionRow& r, long lo, long hi) {
  std::string s = std::string(r.name) + ": " + (r.zero_too ? "0 or " : "");
  s += hi == LONG_MAX ? ">= " + std::to_string(lo) : std::to_string(lo) + ".." + std::to_string(hi);
  if (r.multiple > 1) s += " in multiples of " + std::to_string(r.multiple);
  return s;
}

inline bool crc_ablate_accepts(const OptionRow&, long v, const OptionEnv& env, std::string* why) {
  if (v == 0 || v == 3 || (env.ab_build && v >= 2 && v <= 12)) return true;
  *why = env.ab_build ? "crc_ablate: 0 or 2..12" : "crc_ablate: 0 or 3 (2, 4..12: a library built with the A/B ablations)";
  return false;
}
inline bool wal_pipe_cus_accepts(const OptionRow& r, long v, const OptionEnv& env, std::string* why) {
  if (v >= r.lo && v < env.ncu) return true;
  *why = option_range(r, r.lo, (long)env.ncu - 1) + " (the device's compute units less one)";
  return false;
}
inline void variant_stored(Options& o) {
  o.variant = (o.variant & ~(kVariantAblate | kVariantBatchOrder | kVariantNoStream | kVariantStreamOnly)) |
              (o.crc_ablate << 8) | (o.sha_order ? 0 : kVariantBatchOrder) |
              (o.crc_stream == 0 ? kVariantNoStream : o.crc_stream == 2 ? kVariantStreamOnly : 0);
}

#define LSMCK_OPT(name, ...) {#name, &Options::name, __VA_ARGS__}
constexpr OptionRow kOptions[] = {
    LSMCK_OPT(crc_ablate, 0, 12, false, 1, crc_ablate_accepts, variant_stored),
    LSMCK_OPT(tree_active_files, 0, 1l << 20),
    LSMCK_OPT(tree_slice_bytes, 0, 1l << 30, false, 64),
    LSMCK_OPT(tree_list_batch, 0, 1l << 20),
    LSMCK_OPT(tree_overlap, 0, 1l << 30),
    LSMCK_OPT(tree_json_threads, 0, 64),
    LSMCK_OPT(tree_stages, 2, 3),
    LSMCK_OPT(tree_open_files, -1, LONG_MAX),
    LSMCK_OPT(tree_cpu_file_bytes, 0, LONG_MAX),
    LSMCK_OPT(tree_list_threads, 0, 256),
    LSMCK_OPT(tree_readers, 1, 64),
    LSMCK_OPT(stage_threads, 1, 64),
    LSMCK_OPT(wal_chunk_bytes, 0, LONG_MAX),
    LSMCK_OPT(wal_gpu_walk, 0, 1),
    LSMCK_OPT(wal_stage_bytes, 1l << 20, 64l << 20, false, 64l << 10),
    LSMCK_OPT(wal_part_bytes, 1l << 20, LONG_MAX, true),
    LSMCK_OPT(wal_split, 0, 1),
    LSMCK_OPT(wal_register, 0, 1),
    LSMCK_OPT(wal_upload_min, 0, LONG_MAX),
    LSMCK_OPT(wal_seg_walk, 0, 1),
    LSMCK_OPT(wal_dma_engines, 0, 16),
    LSMCK_OPT(wal_dma_chunks, 1, 64),
    LSMCK_OPT(wal_seg_bytes, 64, 1l << 30, true),
    LSMCK_OPT(stage_numa, -2, 1023),  // (lsmck_ctx_set_option then places the staging anew)
    LSMCK_OPT(wal_seg_stage, 0, 1l << 24),
    LSMCK_OPT(wal_seg_pack, 0, 1),
    LSMCK_OPT(wal_seg_prepair, 0, 64),
    LSMCK_OPT(wal_seg_rounds, 0, 1024),
    LSMCK_OPT(wal_pipe, 0, 64),
    LSMCK_OPT(wal_pipe_first, 1, 63),
    LSMCK_OPT(wal_pipe_cus, 1, LONG_MAX, false, 1, wal_pipe_cus_accepts),
    LSMCK_OPT(wal_pipe_min, 0, LONG_MAX),
    LSMCK_OPT(wal_pipe_seg, 4096, 1l << 30, true),
    LSMCK_OPT(wal_pipe_layout, 0, 1),
    LSMCK_OPT(wal_prefetch, 0, 1l << 24),
    LSMCK_OPT(sha_bucket_from, 2, 1024),
    LSMCK_OPT(sha_bucket_shift, 0, 6),
    LSMCK_OPT(sha_short_blocks, 0, 127),
    LSMCK_OPT(sha_pair, 0, 3),
    LSMCK_OPT(sha_order, 0, 1, false, 1, nullptr, variant_stored),
    LSMCK_OPT(crc_stream, 0, 2, false, 1, nullptr, variant_stored),
    LSMCK_OPT(wal_encode_time, 0, 1),
    LSMCK_OPT(sst_encode_time, 0, 1),
    LSMCK_OPT(mem_build_time, 0, 1),
};
// the batch write plan's rows (lsmck_db_write_plan), looked up behind kOptions
constexpr OptionRow kPlanOptions[] = {
    LSMCK_OPT(cut_walk_cap, 1, 1l << 30),
    LSMCK_OPT(cut_block, 64, 8192),
};
// the opened table set's (lsmck_tableset_open), looked up behind kPlanOptions
constexpr OptionRow kSetOptions[] = {
    LSMCK_OPT(fence_walk_cap, 1, 1l << 20),
    LSMCK_OPT(bloom_bits, 4, 64, true),
};
#undef LSMCK_OPT

// Looks `key` up, checks `value` against its row and stores it.  Returns 0, or
// LSMCK_EINVAL with *why naming the key and the values it takes (nothing stored).
inline int option_set(Options& o, const char* key, long value, const OptionEnv& env, std::string* why) {
  if (!key) return *why = "null key", LSMCK_EINVAL;
  constexpr size_t kRows = sizeof kOptions / sizeof kOptions[0];
  constexpr size_t kPlanRows = sizeof kPlanOptions / sizeof kPlanOptions[0];
  constexpr size_t kSetRows = sizeof kSetOptions / sizeof kSetOptions[0];
  for (size_t i = 0; i < kRows + kPlanRows + kSetRows; ++i) {
    const OptionRow& r = i < kRows               ? kOptions[i]
                         : i < kRows + kPlanRows ? kPlanOptions[i - kRows]
                                                 : kSetOptions[i - kRows - kPlanRows];
    if (strcmp(key, r.name)) continue;
    if (r.accepts) {
      if (!r.accepts(r, value, env, why)) return LSMCK_EINVAL;
    } else if (!((value >= r.lo && value <= r.hi) || (r.zero_too && value == 0)) || value % r.multiple) {
      return *why = option_range(r, r.lo, r.hi), LSMCK_EINVAL;
    }
    o.*r.field = value;
    if (r.stored) r.stored(o);
    return 0;
  }
  return *why = std::string("unknown option: ") + key, LSMCK_EINVAL;
}

}  // namespace lsmck_host
#endif
