// lsmck_buf.h -- the host layer's one owning, grow-only buffer.
//
// GrowBuf<T, Alloc> owns a block of `cap()` elements of T that Alloc gave it
// and frees it when it goes out of scope.  It only ever grows:
//   ensure(need)        nothing when it already holds `need` elements; else the
//                       old block is released FIRST and max(need, cap * 3/2)
//                       elements (at least 1) are allocated -- on a nearly full
//                       device the two blocks never exist side by side.  The
//                       contents are not kept.  On failure the buffer is empty.
//   ensure_keep(...)    the same growth, but the first `keep` elements survive:
//                       the new block is allocated beside the old one, filled
//                       on `stream`, and the old one freed after the copy.  A
//                       failure leaves the old block as it was.
// Both come in two forms: try_*() hands Alloc's own error back untouched (the
// caller may decline and carry on), the plain form turns it into the library's
// return code through Alloc::fail (which also records the message).
//
// Alloc supplies:  err_t;  static bool ok(err_t);  static int fail(err_t);
//   static err_t alloc(void** p, size_t bytes, extra...);   (extra: whatever
//                       ensure() was given after `need`, e.g. a NUMA node)
//   static void free(void* p);
//   static err_t copy(void* dst, const void* src, size_t bytes, stream);
//                       (copy and wait; only ensure_keep uses it)
// The header itself needs nothing from HIP: the device and pinned allocators
// are in lsmck_api.cpp, tests/native/test_growbuf.cpp brings a counting malloc.
#ifndef LSMCK_BUF_H
#define LSMCK_BUF_H
#include <stddef.h>

#include <algorithm>

namespace lsmck_host {

template <typename T, typename Alloc>
class GrowBuf {
 public:
  using err_t = typename Alloc::err_t;
  GrowBuf() = default;
  GrowBuf(const GrowBuf&) = delete;
  GrowBuf& operator=(const GrowBuf&) = delete;
  GrowBuf(GrowBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  GrowBuf& operator=(GrowBuf&& o) noexcept {
    if (this != &o) {
      release();
      p_ = o.p_, cap_ = o.cap_;
      o.p_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  ~GrowBuf() { release(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }  // reads as the pointer it replaces: buf + i, buf[i], f(buf)
  size_t cap() const { return cap_; }
  void release() {
    if (p_) Alloc::free(p_);
    p_ = nullptr;
    cap_ = 0;
  }

  template <typename... Extra>
  err_t try_ensure(size_t need, Extra... extra) {
    if (p_ && cap_ >= need) return err_t{};
    const size_t want = std::max<size_t>(std::max(need, cap_ * 3 / 2), 1);
    release();
    void* q = nullptr;
    const err_t e = Alloc::alloc(&q, want * sizeof(T), extra...);
    if (!Alloc::ok(e)) return e;
    p_ = (T*)q;
    cap_ = want;
    return e;
  }
  template <typename Stream>
  err_t try_ensure_keep(size_t need, size_t keep, Stream stream) {
    if (p_ && cap_ >= need) return err_t{};
    if (!keep || !p_) return try_ensure(need);
    const size_t want = std::max(need, cap_ * 3 / 2);
    void* q = nullptr;
    err_t e = Alloc::alloc(&q, want * sizeof(T));
    if (!Alloc::ok(e)) return e;
    e = Alloc::copy(q, p_, keep * sizeof(T), stream);
    if (!Alloc::ok(e)) {
      Alloc::free(q);
      return e;
    }
    Alloc::free(p_);
    p_ = (T*)q;
    cap_ = want;
    return e;
  }
  template <typename... Extra>
  int ensure(size_t need, Extra... extra) {
    const err_t e = try_ensure(need, extra...);
    return Alloc::ok(e) ? 0 : Alloc::fail(e);
  }
  template <typename Stream>
  int ensure_keep(size_t need, size_t keep, Stream stream) {
    const err_t e = try_ensure_keep(need, keep, stream);
    return Alloc::ok(e) ? 0 : Alloc::fail(e);
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

}  // namespace lsmck_host
#endif
