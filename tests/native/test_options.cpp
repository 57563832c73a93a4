// lsmck_ctx_set_option's table (csrc/lsmck_options.h) against a table written
// out by hand here: every option's default, the values it takes and the ones
// it refuses (nothing stored then), the three options kept as bits of
// `variant`, and the two whose range depends on the device or the build.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>

#include "lsmck_options.h"

using lsmck_host::Options;

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_what); \
      exit(1);                                                              \
    }                                                                       \
  } while (0)
static const char* g_what = "";

constexpr long kNone = LONG_MAX;  // no upper bound
constexpr long MiB = 1l << 20;
struct Want {
  const char* name;
  long Options::*field;
  long dflt, lo, hi;
  bool zero_too;  // 0 is accepted below lo
  long multiple;
};
// (crc_ablate and wal_pipe_cus: their ranges are checked apart, below)
static const Want kWant[] = {
    {"crc_ablate", &Options::crc_ablate, 0, 0, 0, false, 1},
    {"tree_active_files", &Options::tree_active_files, 0, 0, 1l << 20, false, 1},
    {"tree_slice_bytes", &Options::tree_slice_bytes, 0, 0, 1l << 30, false, 64},
    {"tree_list_batch", &Options::tree_list_batch, 0, 0, 1l << 20, false, 1},
    {"tree_overlap", &Options::tree_overlap, 2048, 0, 1l << 30, false, 1},
    {"tree_json_threads", &Options::tree_json_threads, 0, 0, 64, false, 1},
    {"tree_stages", &Options::tree_stages, 3, 2, 3, false, 1},
    {"tree_open_files", &Options::tree_open_files, -1, -1, kNone, false, 1},
    {"tree_cpu_file_bytes", &Options::tree_cpu_file_bytes, 0, 0, kNone, false, 1},
    {"tree_list_threads", &Options::tree_list_threads, 0, 0, 256, false, 1},
    {"tree_readers", &Options::tree_readers, 16, 1, 64, false, 1},
    {"stage_threads", &Options::stage_threads, 8, 1, 64, false, 1},
    {"wal_chunk_bytes", &Options::wal_chunk_bytes, 32 * MiB, 0, kNone, false, 1},
    {"wal_gpu_walk", &Options::wal_gpu_walk, 1, 0, 1, false, 1},
    {"wal_stage_bytes", &Options::wal_stage_bytes, 16 * MiB, 1 * MiB, 64 * MiB, false, 64 << 10},
    {"wal_part_bytes", &Options::wal_part_bytes, 0, 1 * MiB, kNone, true, 1},
    {"wal_split", &Options::wal_split, 1, 0, 1, false, 1},
    {"wal_register", &Options::wal_register, 0, 0, 1, false, 1},
    {"wal_upload_min", &Options::wal_upload_min, 1 * MiB, 0, kNone, false, 1},
    {"wal_seg_walk", &Options::wal_seg_walk, 1, 0, 1, false, 1},
    {"wal_dma_engines", &Options::wal_dma_engines, 4, 0, 16, false, 1},
    {"wal_dma_chunks", &Options::wal_dma_chunks, 32, 1, 64, false, 1},
    {"wal_seg_bytes", &Options::wal_seg_bytes, 0, 64, 1l << 30, true, 1},
    {"stage_numa", &Options::stage_numa, -2, -2, 1023, false, 1},
    {"wal_seg_stage", &Options::wal_seg_stage, 1, 0, 1l << 24, false, 1},
    {"wal_seg_pack", &Options::wal_seg_pack, 1, 0, 1, false, 1},
    {"wal_seg_prepair", &Options::wal_seg_prepair, 2, 0, 64, false, 1},
    {"wal_seg_rounds", &Options::wal_seg_rounds, 16, 0, 1024, false, 1},
    {"wal_pipe", &Options::wal_pipe, 0, 0, 64, false, 1},
    {"wal_pipe_first", &Options::wal_pipe_first, 4, 1, 63, false, 1},
    {"wal_pipe_cus", &Options::wal_pipe_cus, 32, 1, 255, false, 1},  // (ncu 256 below)
    {"wal_pipe_min", &Options::wal_pipe_min, 1l << 30, 0, kNone, false, 1},
    {"wal_pipe_seg", &Options::wal_pipe_seg, 0, 4096, 1l << 30, true, 1},
    {"wal_pipe_layout", &Options::wal_pipe_layout, 0, 0, 1, false, 1},
    {"wal_prefetch", &Options::wal_prefetch, 4096, 0, 1l << 24, false, 1},
    {"sha_bucket_from", &Options::sha_bucket_from, 128, 2, 1024, false, 1},
    {"sha_bucket_shift", &Options::sha_bucket_shift, 2, 0, 6, false, 1},
    {"sha_short_blocks", &Options::sha_short_blocks, 12, 0, 127, false, 1},
    {"sha_pair", &Options::sha_pair, 1, 0, 3, false, 1},
    {"sha_order", &Options::sha_order, 1, 0, 1, false, 1},
    {"crc_stream", &Options::crc_stream, 1, 0, 2, false, 1},
    {"wal_encode_time", &Options::wal_encode_time, 0, 0, 1, false, 1},
    {"sst_encode_time", &Options::sst_encode_time, 0, 0, 1, false, 1},
    {"mem_build_time", &Options::mem_build_time, 0, 0, 1, false, 1},
};
constexpr size_t kCount = sizeof kWant / sizeof kWant[0];

static const lsmck_host::OptionEnv kEnv{256, false}, kEnvAB{256, true};

static void accept(Options& o, const Want& w, long v, const lsmck_host::OptionEnv& env = kEnv) {
  std::string why;
  CHECK(lsmck_host::option_set(o, w.name, v, env, &why) == 0);
  CHECK(o.*w.field == v && why.empty());
}
static void refuse(Options& o, const Want& w, long v, const lsmck_host::OptionEnv& env = kEnv) {
  const long before = o.*w.field, variant = o.variant;
  std::string why;
  CHECK(lsmck_host::option_set(o, w.name, v, env, &why) == LSMCK_EINVAL);
  CHECK(o.*w.field == before && o.variant == variant);
  CHECK(why.find(w.name) != std::string::npos);  // the message names the key
}

int main() {
  // the table: every option once, none besides
  CHECK(sizeof lsmck_host::kOptions / sizeof lsmck_host::kOptions[0] == kCount);
  std::set<std::string> names, wanted;
  for (const auto& r : lsmck_host::kOptions) CHECK(names.insert(r.name).second);
  for (const Want& w : kWant) CHECK(wanted.insert(w.name).second);
  CHECK(names == wanted);
  {
    const Options o{};
    for (const Want& w : kWant) {
      g_what = w.name;
      CHECK(o.*w.field == w.dflt);
    }
    CHECK(o.variant == 0);
  }
  for (const Want& w : kWant) {
    g_what = w.name;
    if (!strcmp(w.name, "crc_ablate")) continue;
    Options o{};
    const long m = w.multiple;
    accept(o, w, w.lo);
    accept(o, w, w.hi == kNone ? (1l << 40) : w.hi);
    if (w.hi == kNone) accept(o, w, kNone);
    if (m > 1) accept(o, w, w.lo + m);
    if (m > 1 || w.hi == kNone || w.hi - w.lo >= 2) accept(o, w, w.lo + (m > 1 ? 2 * m : 1));  // (an interior value)
    refuse(o, w, w.lo - 1);
    if (w.hi != kNone) refuse(o, w, w.hi + 1);
    if (m > 1) {
      refuse(o, w, w.lo + 1);
      refuse(o, w, w.lo + m / 2);
      refuse(o, w, w.hi - 1);
    }
    if (w.zero_too) {
      accept(o, w, 0);
      refuse(o, w, -1);
      refuse(o, w, 1);
    }
    refuse(o, w, LONG_MIN);
  }
  g_what = "crc_ablate";
  {
    const Want& w = kWant[0];
    Options o{};
    for (long v : {0l, 3l}) accept(o, w, v);
    for (long v : {-1l, 1l, 2l, 4l, 12l, 13l}) refuse(o, w, v);
    for (long v = 2; v <= 12; ++v) accept(o, w, v, kEnvAB);
    accept(o, w, 0, kEnvAB);
    for (long v : {-1l, 1l, 13l}) refuse(o, w, v, kEnvAB);
  }
  g_what = "wal_pipe_cus";
  {
    Options o{};
    std::string why;
    CHECK(lsmck_host::option_set(o, "wal_pipe_cus", 255, {256, false}, &why) == 0 && o.wal_pipe_cus == 255);
    CHECK(lsmck_host::option_set(o, "wal_pipe_cus", 256, {256, false}, &why) == LSMCK_EINVAL && o.wal_pipe_cus == 255);
    CHECK(lsmck_host::option_set(o, "wal_pipe_cus", 255, {255, false}, &why) == LSMCK_EINVAL);
    CHECK(lsmck_host::option_set(o, "wal_pipe_cus", 303, {304, false}, &why) == 0 && o.wal_pipe_cus == 303);
  }
  g_what = "variant";
  {
    Options o{};
    std::string why;
    auto set = [&](const char* k, long v) { CHECK(lsmck_host::option_set(o, k, v, kEnv, &why) == 0); };
    set("crc_stream", 0);
    CHECK(o.variant == 0x200000);
    set("crc_stream", 1);
    CHECK(o.variant == 0);
    set("crc_stream", 2);
    CHECK(o.variant == 0x400000);
    set("crc_stream", 1);
    set("sha_order", 0);
    CHECK(o.variant == 0x10000);
    set("sha_order", 1);
    CHECK(o.variant == 0);
    // the ablation field beside the other bits, each kept when another changes
    set("sha_order", 0);
    set("crc_stream", 0);
    set("crc_ablate", 3);
    CHECK(o.variant == (0x300 | 0x10000 | 0x200000));
    CHECK((o.variant & 0xF00) == 0x300);
    set("crc_stream", 2);
    CHECK(o.variant == (0x300 | 0x10000 | 0x400000));
    set("crc_ablate", 0);
    set("sha_order", 1);
    CHECK(o.variant == 0x400000);
    // a plain option leaves it alone
    set("sha_pair", 0);
    CHECK(o.variant == 0x400000);
  }
  g_what = "keys";
  {
    Options o{};
    std::string why;
    CHECK(lsmck_host::option_set(o, "no_such_option", 1, kEnv, &why) == LSMCK_EINVAL && !why.empty());
    CHECK(lsmck_host::option_set(o, "", 1, kEnv, &why) == LSMCK_EINVAL);
    CHECK(lsmck_host::option_set(o, "variant", 1, kEnv, &why) == LSMCK_EINVAL);  // (a field, not an option)
    CHECK(lsmck_host::option_set(o, nullptr, 1, kEnv, &why) == LSMCK_EINVAL && !why.empty());
  }
  printf("options ok (%zu)\n", kCount);
  return 0;
}
