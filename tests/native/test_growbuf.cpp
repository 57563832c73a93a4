// The host layer's owning buffer (csrc/lsmck_buf.h) over a counting malloc that
// can be told to fail its k-th allocation: the growth rule, the order of free
// and allocate, what a failure leaves behind, ensure_keep, moves, and that
// every block is freed exactly once.  Blocks are exact-size mallocs, so the
// sanitizer sees any access past one.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "lsmck_buf.h"

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

struct Counting {
  using err_t = int;
  static constexpr int kNoMem = -12;
  static std::vector<std::string> log;  // "a<bytes>" / "f" in call order
  static long live, allocs, frees, fail_at;  // fail_at: the allocation (1-based, counted from reset) that fails
  static int last_extra;
  static void reset(long fail = 0) {
    log.clear();
    allocs = frees = 0;
    fail_at = fail;
  }
  static bool ok(int e) { return e == 0; }
  static int fail(int e) { return e; }
  static int alloc(void** p, size_t bytes, int extra = 0) {
    ++allocs;
    log.push_back("a" + std::to_string(bytes));
    last_extra = extra;
    if (allocs == fail_at) return kNoMem;
    *p = malloc(bytes);
    ++live;
    return 0;
  }
  static void free(void* p) {
    ++frees;
    --live;
    log.push_back("f");
    ::free(p);
  }
  static int copy(void* dst, const void* src, size_t bytes, int) {
    memcpy(dst, src, bytes);
    return 0;
  }
};
std::vector<std::string> Counting::log;
long Counting::live = 0, Counting::allocs = 0, Counting::frees = 0, Counting::fail_at = 0;
int Counting::last_extra = 0;

using Buf = lsmck_host::GrowBuf<uint32_t, Counting>;

int main() {
  {
    Buf b;
    CHECK(b.get() == nullptr && b.cap() == 0);
    Counting::reset();
    CHECK(b.ensure(0) == 0);  // an empty buffer asked for nothing: one element
    CHECK(b.cap() == 1 && b.get() && Counting::allocs == 1 && Counting::log[0] == "a4");
    b[0] = 7;
    // within the capacity: no allocator call
    Counting::reset();
    CHECK(b.ensure(1) == 0 && b.ensure(0) == 0);
    CHECK(Counting::allocs == 0 && Counting::frees == 0 && b.cap() == 1);
    // 10, then 11 -> 15 (3/2 of 10), then 100 (the need, above 3/2 of 15)
    CHECK(b.ensure(10) == 0 && b.cap() == 10);
    Counting::reset();
    CHECK(b.ensure(10) == 0 && Counting::allocs == 0);
    CHECK(b.ensure(11) == 0 && b.cap() == 15);
    // the old block goes before the new one is asked for
    CHECK(Counting::log.size() == 2 && Counting::log[0] == "f" && Counting::log[1] == "a60");
    for (size_t i = 0; i < b.cap(); ++i) b[i] = (uint32_t)i;  // (every element is there)
  }
  CHECK(Counting::live == 0);  // the destructor freed it
  {
    Buf b;
    CHECK(b.ensure(10) == 0 && b.cap() == 10);
    CHECK(b.ensure(100) == 0 && b.cap() == 100);
    // a failed growth: empty, the allocator's error, and the next one works
    Counting::reset(1);
    CHECK(b.ensure(101) == Counting::kNoMem);
    CHECK(b.get() == nullptr && b.cap() == 0);
    CHECK(Counting::log.size() == 2 && Counting::log[0] == "f" && Counting::log[1] == "a600");  // 150 elements asked for
    CHECK(Counting::live == 0);
    Counting::reset();
    CHECK(b.try_ensure(5) == 0 && b.cap() == 5 && b.get());  // (from empty: the need itself)
    // the extra argument reaches the allocator
    CHECK(b.ensure(6, 42) == 0 && Counting::last_extra == 42 && b.cap() == 7);
  }
  CHECK(Counting::live == 0);
  {  // ensure_keep: the first `keep` elements survive, the rest of the new block is left alone
    Buf b;
    CHECK(b.ensure_keep(4, 3, 0) == 0 && b.cap() == 4);  // empty: plain ensure
    for (uint32_t i = 0; i < 4; ++i) b[i] = 100 + i;
    Counting::reset();
    CHECK(b.ensure_keep(4, 4, 0) == 0 && Counting::allocs == 0);  // it fits: nothing
    CHECK(b.ensure_keep(5, 3, 0) == 0 && b.cap() == 6);            // max(5, 4 * 3/2)
    CHECK(Counting::log.size() == 2 && Counting::log[0] == "a24" && Counting::log[1] == "f");  // new first, then the old one
    CHECK(b[0] == 100 && b[1] == 101 && b[2] == 102);
    for (uint32_t i = 3; i < 6; ++i) b[i] = i;  // (writable up to the new capacity)
    // a failed ensure_keep keeps the block it had
    Counting::reset(1);
    const uint32_t* before = b.get();
    CHECK(b.ensure_keep(7, 6, 0) == Counting::kNoMem);
    CHECK(b.get() == before && b.cap() == 6 && b[0] == 100 && b[5] == 5 && Counting::frees == 0);
    // keep == 0: plain ensure (free first)
    Counting::reset();
    CHECK(b.ensure_keep(7, 0, 0) == 0 && b.cap() == 9);
    CHECK(Counting::log.size() == 2 && Counting::log[0] == "f" && Counting::log[1] == "a36");
  }
  CHECK(Counting::live == 0);
  {  // moves: the source frees nothing, the target frees once
    Buf a;
    CHECK(a.ensure(8) == 0);
    uint32_t* p = a.get();
    Buf b(std::move(a));
    CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == p && b.cap() == 8);
    Buf c;
    CHECK(c.ensure(2) == 0);
    Counting::reset();
    c = std::move(b);  // c's own block goes, b's moves in
    CHECK(Counting::frees == 1 && Counting::allocs == 0 && c.get() == p && c.cap() == 8 && b.get() == nullptr);
    Counting::reset();
    { Buf gone(std::move(a)); }  // a moved-from buffer, moved again and destroyed: nothing to free
    CHECK(Counting::frees == 0);
    c.release();
    CHECK(Counting::frees == 1 && c.get() == nullptr && c.cap() == 0);
    c.release();
    CHECK(Counting::frees == 1);
  }
  CHECK(Counting::live == 0);
  printf("growbuf ok\n");
  return 0;
}
