// lsmck_splan.h -- the stream kernel's slice plan (crc32_stream_kernel,
// lsmck_crc32.hip): how many slices a batch is cut into and where on the byte
// axis the cuts lie.  Shared by the cut pass (stream_cut, device), the
// launcher (host) and the host test of the plan (tests/native/splan_export.cpp,
// plain C++).  Internal to liblsmck.so.
//
// The waves of a CU run equal shares at paces about 8 % apart, so a wave that
// is done early should go on with work the late ones would be left with --
// but every slice costs its wave a restart, and what the waves lose at the
// end is about half of the LAST slices' time.  So the plan spends its slices
// where they shorten the tail:
//  * a first region of one large slice per wave (slice `wave`, taken without
//    a ticket), STREAM_PLAN_F0 percent of the bytes;
//  * a ticketed region of groups of W slices in ticket order; a group's slice
//    is STREAM_PLAN_R percent of the group's before, down to the first
//    group's size >> STREAM_PLAN_FLOOR.
// A batch of fewer slices (stream_slices: at least 64 records a slice) uses
// the first groups only, and the first region is never cut finer than the
// first ticket group: at one ticket group the slices are nearly equal, at
// one slice per wave equal.  (R = 100, F0 = 0: equal slices, the A/B control.)
#ifndef LSMCK_SPLAN_H
#define LSMCK_SPLAN_H
#include <stdint.h>

#if defined(__HIPCC__)
#define LSMCK_SPLAN_HD __host__ __device__
#else
#define LSMCK_SPLAN_HD
#endif

#ifndef STREAM_SLICES
#define STREAM_SLICES 16u  // slices per wave on a large batch
#endif
// The fractions were chosen by measurement (profiles/r08/handover):
// 72 % in the first region, ticket groups of 8 : 4 : 2 : 1 : 1 ... -- on config
// 3 (3,120 tiles a wave) first slices of 2,246 tiles, ticketed ones of 269
// down to 34.  A larger first region runs faster on some devices and falls
// off a cliff on others (from 84 % on: the slowest waves' first slices then
// end after everything else); 72 % leaves a wave 39 % of slack in its pace.
#ifndef STREAM_PLAN_F0
#define STREAM_PLAN_F0 72u
#endif
#ifndef STREAM_PLAN_R
#define STREAM_PLAN_R 50u
#endif
#ifndef STREAM_PLAN_FLOOR
#define STREAM_PLAN_FLOOR 3u
#endif

static_assert(STREAM_SLICES >= 1u && STREAM_SLICES <= 64u, "slices per wave");
static_assert(STREAM_PLAN_F0 < 100u, "the first region's share is a percentage under 100");
static_assert(STREAM_PLAN_R >= 1u && STREAM_PLAN_R <= 100u, "a ticket group is no larger than the one before");
static_assert(STREAM_PLAN_FLOOR <= 20u, "the floor is a shift of the first group's 2^20");

namespace lsmck {
namespace splan {

// waves of a launch: 16 per CU (one 1024-thread workgroup each)
LSMCK_SPLAN_HD inline uint32_t waves(int ncu) { return (uint32_t)ncu * 16u; }
LSMCK_SPLAN_HD inline uint32_t slices_max(int ncu) { return waves(ncu) * STREAM_SLICES; }

// slices of a batch of n records: one per wave, and from 64 records per slice
// on more, up to STREAM_SLICES per wave
LSMCK_SPLAN_HD inline uint32_t slices(int ncu, uint64_t n) {
  const uint64_t w = waves(ncu), hi = w * STREAM_SLICES, by_rec = n / 64u;
  const uint64_t s = by_rec > w ? by_rec : w;
  return (uint32_t)(s < hi ? s : hi);
}

// weight of a slice of ticket group g (the first group's: 2^20)
LSMCK_SPLAN_HD inline uint64_t group_weight(uint32_t g) {
  const uint64_t lo = (1u << 20) >> STREAM_PLAN_FLOOR;
  uint64_t w = 1u << 20;
  for (uint32_t i = 0; i < g && w > lo; ++i) w = w * STREAM_PLAN_R / 100u;
  return w > lo ? w : lo;
}

// weight of the first t ticketed slices (groups of W)
LSMCK_SPLAN_HD inline uint64_t ticket_prefix(uint32_t t, uint32_t W) {
  uint64_t p = 0;
  uint32_t g = 0;
  for (; t >= W; t -= W, ++g) p += (uint64_t)W * group_weight(g);
  return p + (uint64_t)t * group_weight(g);
}

// The plan: the byte fraction at which cut s lies, s = 0..S, of a batch cut
// into S slices for W waves (S >= W).  Integer weights, so the fractions are
// exactly monotone and the slice sizes exactly non-increasing before the one
// division.
LSMCK_SPLAN_HD inline double fraction(uint32_t s, uint32_t S, uint32_t W) {
  if (s >= S) return 1.0;
  if (S <= W) return (double)s / (double)S;  // one slice per wave: equal shares
  const uint64_t tk = ticket_prefix(S - W, W);
  uint64_t first = (STREAM_PLAN_F0 * tk + (100u - STREAM_PLAN_F0) * W - 1u) / ((100u - STREAM_PLAN_F0) * W);
  if (first < (1u << 20)) first = 1u << 20;
  const uint64_t total = first * W + tk;
  const uint64_t p = s <= W ? first * s : first * W + ticket_prefix(s - W, W);
  return (double)p / (double)total;
}

}  // namespace splan
}  // namespace lsmck
#endif
