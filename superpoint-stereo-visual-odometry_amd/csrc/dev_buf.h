// dev_buf.h -- the buffers that grow on demand: an owning pointer (Buf) and the one protocol that re-allocates a list of them
// (grow_list).  Plain C++17 without a HIP include: where memory comes from is a policy parameter -- the library's two are in
// spvo_internal.hip.h (device and pinned host memory) -- so the same code builds into a stand-alone program with a counting fake
// policy that runs under the sanitizers on the CPU (tools/dev_buf_check.cpp, tests/test_dev_buf_cpu.py).
//
// A policy P has
//   static int alloc(void **p, size_t bytes)                     0, or its own error code
//   static void release(void *p)
//   static constexpr const char *alloc_call                      the name an error text gives alloc
// and, if any of its buffers is asked to be cleared,
//   static int clear(void *p, size_t bytes, void *where)         zeroes the block, possibly asynchronously on `where`; 0 or a code
//   static constexpr const char *clear_call
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace spvo_int {

// One buffer of `count()` values of T and nothing else: frees in its destructor and in reset(), moves, does not copy, and reads as
// the T * it owns wherever one is expected.  A deduced template parameter or a `cond ? buf : nullptr` needs get().
template <class T, class P>
class Buf {
  T *p_ = nullptr;
  size_t n_ = 0;

 public:
  Buf() = default;
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  Buf &operator=(Buf &&o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
    return *this;
  }
  ~Buf() { reset(); }
  void reset() {
    if (p_) P::release(p_);
    p_ = nullptr; n_ = 0;
  }
  // a fresh block for `count` values (one at least, so that a buffer that exists is never NULL), the old one freed first
  int alloc(size_t count) {
    reset();
    void *p = nullptr;
    if (int e = P::alloc(&p, (count ? count : 1) * sizeof(T))) return e;
    p_ = static_cast<T *>(p); n_ = count;
    return 0;
  }
  operator T *() const { return p_; }
  T *get() const { return p_; }
  size_t count() const { return n_; }
  size_t bytes() const { return (n_ ? n_ : 1) * sizeof(T); }
};

// one entry of a grow list: this buffer, that many values, zeroed (Clear) or not (grow_entry fills the two functions in)
struct GrowEntry {
  void *buf;
  size_t count;
  bool clear;
  void (*reset)(void *buf);
  int (*alloc)(const GrowEntry &e, void *where, const char **call);
};
template <bool Clear, class T, class P>
GrowEntry grow_entry(Buf<T, P> &b, size_t count) {
  return GrowEntry{&b, count, Clear, [](void *buf) { static_cast<Buf<T, P> *>(buf)->reset(); },
                   [](const GrowEntry &e, void *where, const char **call) {
                     Buf<T, P> &o = *static_cast<Buf<T, P> *>(e.buf);
                     *call = P::alloc_call;
                     if (int err = o.alloc(e.count)) return err;
                     if constexpr (Clear) {
                       *call = P::clear_call;
                       return P::clear(o.get(), o.bytes(), where);
                     } else {
                       (void)where;
                       return 0;
                     }
                   }};
}

struct GrowResult {
  int code = 0;                 // 0, or the failing call's error code ...
  const char *call = nullptr;   // ... and its name
  bool cleared = false;         // a clearing was enqueued on `where`: the caller waits for it before it hands the buffers out
};

// The grow protocol behind its wait: every buffer of the list is freed, then every one allocated (and cleared on `where`, if asked), in
// the list's order.  The first failure frees what this call allocated: all of the list is empty then, so that what owns the buffers
// can still be destroyed and a later call can grow them again.
inline GrowResult grow_list(const std::vector<GrowEntry> &list, void *where) {
  GrowResult r;
  for (const GrowEntry &e : list) e.reset(e.buf);
  for (const GrowEntry &e : list) {
    if ((r.code = e.alloc(e, where, &r.call))) {
      for (const GrowEntry &f : list) f.reset(f.buf);
      return r;
    }
    r.cleared |= e.clear;
  }
  r.call = nullptr;
  return r;
}

}  // namespace spvo_int
