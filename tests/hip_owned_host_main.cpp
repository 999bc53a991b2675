// Driver of tests/test_hip_owned_host.py: the ownership and growth logic of
// ekf-slam_amd/csrc/hip_owned.hpp on the CPU. The generic part of the header alone
// (HIP_OWNED_NO_HIP: no HIP header, no HIP runtime) is instantiated with a counting allocator that
// fails on request, once in the manner of DeviceBuf (no flags) and once in the manner of PinnedBuf
// (flags handed through to the allocator). Built with ASan + UBSan; exits non-zero at the first
// check that fails.
#define HIP_OWNED_NO_HIP
#include "hip_owned.hpp"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

namespace {

int g_failed = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                      \
    }                                                                  \
  } while (0)

// Counts what the buffers do; `fail_at` = k ≥ 0 makes the k-th alloc from now on return null.
template <int Tag>
struct Fake {
  static inline std::set<void*> live;
  static inline long allocs = 0, frees = 0, bad_frees = 0, cleared = 0, fail_at = -1;
  static inline size_t last_bytes = 0;
  static inline unsigned last_flags = 0;
  static void* alloc(size_t bytes, unsigned flags) {
    last_bytes = bytes;
    last_flags = flags;
    if (fail_at >= 0 && fail_at-- == 0) return nullptr;
    ++allocs;
    void* p = std::malloc(bytes ? bytes : 1);
    live.insert(p);
    return p;
  }
  static void free(void* p) {
    ++frees;
    if (!live.erase(p)) {  // not ours, or freed twice
      ++bad_frees;
      return;
    }
    std::free(p);
  }
  static void clear_error() { ++cleared; }
};

struct Rec {
  double v[5];
};

template <typename A>
void reserve_semantics(unsigned flags) {
  using ekfslam::Buf;
  Buf<Rec, A> b = flags ? Buf<Rec, A>(flags) : Buf<Rec, A>();
  CHECK(b.get() == nullptr && b.capacity() == 0);
  CHECK(b.reserve(0) == EKF_OK && A::allocs == 0);  // nothing asked for, nothing allocated
  // first growth: one block of max(n, at_least)
  CHECK(b.reserve(10) == EKF_OK && b.capacity() == 10 && b.get() != nullptr);
  CHECK(A::allocs == 1 && A::frees == 0 && A::last_bytes == 10 * sizeof(Rec));
  CHECK(A::last_flags == flags);
  b.get()[9].v[4] = 1.0;  // (ASan: the block really holds 10)
  // within capacity: no allocation, the pointer stays; at_least alone never grows
  Rec* p0 = b.get();
  for (size_t n : {size_t{0}, size_t{1}, size_t{10}}) {
    CHECK(b.reserve(n) == EKF_OK && b.reserve(n, 1000) == EKF_OK);
    CHECK(b.get() == p0 && b.capacity() == 10 && A::allocs == 1 && A::frees == 0);
  }
  // beyond: the old block freed exactly once, one new block
  CHECK(b.reserve(11, 20) == EKF_OK && b.capacity() == 20);
  CHECK(A::allocs == 2 && A::frees == 1 && A::last_bytes == 20 * sizeof(Rec));
  CHECK(b.reserve(50, 40) == EKF_OK && b.capacity() == 50);
  CHECK(A::allocs == 3 && A::frees == 2 && A::live.size() == 1);
  b.get()[49].v[0] = 2.0;
  // a failed allocation: empty, EKF_E_NOMEM, the last error cleared, the old block gone once
  A::fail_at = 0;
  const long cleared0 = A::cleared;
  CHECK(b.reserve(51) == EKF_E_NOMEM);
  CHECK(b.get() == nullptr && b.capacity() == 0);
  CHECK(A::cleared == cleared0 + 1 && A::frees == 3 && A::live.empty());
  // ... and a size that fitted before allocates again (no stale capacity)
  CHECK(b.reserve(5) == EKF_OK && b.get() != nullptr && b.capacity() == 5 && A::allocs == 4);
  b.get()[4].v[0] = 3.0;
  // reset: empty, idempotent
  b.reset();
  b.reset();
  CHECK(b.get() == nullptr && b.capacity() == 0 && A::frees == 4 && A::live.empty());
  // bytes for Buf<void>
  Buf<void, A> raw = flags ? Buf<void, A>(flags) : Buf<void, A>();
  CHECK(raw.reserve(77) == EKF_OK && raw.capacity() == 77 && A::last_bytes == 77);
}

// ensure_plan_state, ensure_am, stage_odom, the ring and the simulator's reserve: several buffers
// that are there together or not at all, guarded by the one reserved last.
template <typename A, int K>
struct Group {
  ekfslam::Buf<Rec, A> m[K];
  int reserve(size_t n) {
    if (n <= m[K - 1].capacity()) return EKF_OK;
    for (auto& b : m)
      if (b.reserve(n, 8)) {
        for (auto& o : m) o.reset();
        return EKF_E_NOMEM;
      }
    return EKF_OK;
  }
};

template <typename A>
void all_or_nothing() {
  constexpr int K = 5;
  for (int grown = 0; grown < 2; ++grown)  // from empty, and from a smaller healthy group
    for (int k = 0; k < K; ++k) {
      Group<A, K> g;
      if (grown) CHECK(g.reserve(4) == EKF_OK);
      const size_t n = grown ? 100 : 3;
      A::fail_at = k;
      CHECK(g.reserve(n) == EKF_E_NOMEM);
      CHECK(A::fail_at < 0);  // (the k-th allocation was reached)
      for (auto& b : g.m) CHECK(b.get() == nullptr && b.capacity() == 0);
      CHECK(A::live.empty());
      CHECK(g.reserve(n) == EKF_OK);  // healthy again: every member is there
      for (auto& b : g.m) {
        CHECK(b.get() != nullptr && b.capacity() >= n);
        b.get()[n - 1].v[0] = 1.0;
      }
      const long a0 = A::allocs;
      CHECK(g.reserve(n) == EKF_OK && A::allocs == a0);
    }
  // reset_all, as the call sites use it: `if (a.reserve() || b.reserve()) return reset_all(a, b);`
  for (int k = 0; k < 3; ++k) {
    ekfslam::Buf<Rec, A> a, b;
    ekfslam::Buf<int, A> c;
    A::fail_at = k;
    int rc = EKF_OK;
    if (a.reserve(6) || b.reserve(7) || c.reserve(8)) rc = ekfslam::reset_all(a, b, c);
    CHECK(rc == EKF_E_NOMEM && !a.get() && !b.get() && !c.get() && A::live.empty());
    CHECK(!a.capacity() && !b.capacity() && !c.capacity());
    CHECK(!(a.reserve(6) || b.reserve(7) || c.reserve(8)) && a.get() && b.get() && c.get());
  }
}

template <typename A>
void move_semantics() {
  using B = ekfslam::Buf<Rec, A>;
  B a;
  CHECK(a.reserve(12) == EKF_OK);
  Rec* p = a.get();
  const long frees0 = A::frees;
  B b(std::move(a));  // construction: ownership moves, the source is empty
  CHECK(b.get() == p && b.capacity() == 12 && a.get() == nullptr && a.capacity() == 0);
  B c;
  CHECK(c.reserve(3) == EKF_OK);
  c = std::move(b);  // assignment: the target's own block is freed, once
  CHECK(c.get() == p && c.capacity() == 12 && b.get() == nullptr && b.capacity() == 0);
  CHECK(A::frees == frees0 + 1 && A::live.size() == 1);
  c = std::move(b);  // from an empty source: c is emptied (ekf_trace_enable(0))
  CHECK(c.get() == nullptr && c.capacity() == 0 && A::live.empty());
  CHECK(a.reserve(2) == EKF_OK && a.get() != nullptr);  // a moved-from buffer is an empty one
  B& self = a;
  a = std::move(self);
  CHECK(a.get() != nullptr && a.capacity() == 2);
}

template <typename A>
void run_all(unsigned flags, const char* name) {
  reserve_semantics<A>(flags);
  all_or_nothing<A>();
  move_semantics<A>();
  // exit: every buffer above has gone out of scope
  CHECK(A::live.empty());
  CHECK(A::bad_frees == 0);
  CHECK(A::allocs == A::frees);
  std::printf("%s: %ld allocations, %ld frees, %ld failures cleared\n", name, A::allocs, A::frees,
              A::cleared);
}

}  // namespace

int main() {
  run_all<Fake<0>>(0, "device-style");
  run_all<Fake<1>>(0x6u, "pinned-style");  // (any flags: the allocator must see them)
  if (g_failed) std::fprintf(stderr, "%d checks failed\n", g_failed);
  return g_failed ? 1 : 0;
}
