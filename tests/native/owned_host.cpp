// owned_host.cpp -- csrc/kdpt_owned.h on the host, against a counting stub of the HIP entry points it uses
// (tests/test_sanitizers.py builds this with ASan + UBSan and plain g++).  Every resource the stub hands out is a
// heap block of its own, so a release that is missing shows as a leak, a second release as a double free, and the
// stub's own books (live set, release log) say which.
//
// Checked: every creation is released exactly once -- construction, move-construction, move-assignment onto a
// live handle, self-move, reset, re-creation on a live handle; an arena releases last first; a failed n-th
// allocation leaves the earlier ones owned and released at the end of the scope; a zero-length request allocates
// one element; the masked stream falls back to a plain one; nothing is released twice and nothing is left.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <type_traits>
#include <vector>

// ---- the stub -------------------------------------------------------------------------------------------------
typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1;
typedef struct StubStream* hipStream_t;
typedef struct StubEvent* hipEvent_t;
constexpr unsigned hipHostMallocDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1,
                   hipHostRegisterDefault = 0;

struct Stub {
  std::set<void*> live;         // every resource handed out and not yet released
  std::set<void*> registered;   // hipHostRegister ranges
  std::vector<void*> released;  // in order
  std::vector<size_t> bytes;    // of every device / pinned allocation, in order
  int created = 0, bad_release = 0, masked_streams = 0, plain_streams = 0, timed_events = 0, untimed_events = 0;
  int fail_at = 0;              // fail the n-th creation from now (1 = the next); 0 = none
  bool fail_all = false;        // ... or every one
  bool refuse_masks = false;
  void* make(size_t n) {
    if (fail_all || (fail_at && --fail_at == 0)) return nullptr;
    void* p = malloc(n ? n : 1);
    live.insert(p);
    created++;
    return p;
  }
  hipError_t drop(void* p) {
    if (!live.erase(p)) {
      bad_release++;
      return hipErrorInvalidValue;
    }
    released.push_back(p);
    free(p);
    return hipSuccess;
  }
} g;

hipError_t hipMalloc(void** p, size_t n) {
  g.bytes.push_back(n);
  return (*p = g.make(n)) ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p) { return g.drop(p); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) {
  g.bytes.push_back(n);
  return (*p = g.make(n)) ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* p) { return g.drop(p); }
hipError_t hipEventCreate(hipEvent_t* e) {
  g.timed_events++;
  return (*e = (hipEvent_t)g.make(1)) ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
  g.untimed_events++;
  return (*e = (hipEvent_t)g.make(1)) ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipEventDestroy(hipEvent_t e) { return g.drop(e); }
hipError_t hipExtStreamCreateWithCUMask(hipStream_t* s, uint32_t, const uint32_t*) {
  if (g.refuse_masks) return hipErrorInvalidValue;
  g.masked_streams++;
  return (*s = (hipStream_t)g.make(1)) ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
  g.plain_streams++;
  return (*s = (hipStream_t)g.make(1)) ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipStreamDestroy(hipStream_t s) { return g.drop(s); }
hipError_t hipHostRegister(void* p, size_t, unsigned) {
  return g.registered.insert(p).second ? hipSuccess : hipErrorInvalidValue;
}
hipError_t hipHostUnregister(void* p) {
  if (!g.registered.erase(p)) g.bad_release++;
  return hipSuccess;
}
hipError_t hipGetLastError() { return hipSuccess; }

#define KDPT_OWNED_HIP_STUB
#include "../../kdtreepathtraceroptimization_amd/csrc/kdpt_owned.h"

using namespace kdpt;

// move-only handles, an arena and a registration list that stay where they are
static_assert(!std::is_copy_constructible<DeviceBuf<int>>::value && !std::is_copy_assignable<DeviceBuf<int>>::value &&
                  std::is_nothrow_move_constructible<DeviceBuf<int>>::value, "DeviceBuf");
static_assert(!std::is_copy_constructible<PinnedBuf<int>>::value && !std::is_copy_constructible<Event>::value &&
                  !std::is_copy_constructible<Stream>::value && !std::is_copy_assignable<Event>::value &&
                  !std::is_copy_assignable<Stream>::value, "PinnedBuf, Event, Stream");
static_assert(!std::is_copy_constructible<Arena>::value && !std::is_move_constructible<Arena>::value &&
                  !std::is_copy_constructible<HostRegistrations>::value, "Arena, HostRegistrations");

static int failures = 0;
#define CHECK(x)                                                 \
  do {                                                           \
    if (!(x)) {                                                  \
      failures++;                                                \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #x); \
    }                                                            \
  } while (0)

// every creation so far has been released, exactly once
static void check_balanced() {
  CHECK(g.live.empty());
  CHECK(g.registered.empty());
  CHECK((int)g.released.size() == g.created);
  CHECK(g.bad_release == 0);
}

template <typename H, typename Make>
static void handle_cases(Make make) {
  {  // construction, and a default handle that holds nothing
    H a, none;
    CHECK(!a && !none);
    CHECK(make(a) == hipSuccess && a && a.get());
  }
  check_balanced();
  {  // move-construction: one owner, one release
    H a;
    make(a);
    const auto raw = a.get();
    H b(std::move(a));
    CHECK(!a && b.get() == raw);
  }
  check_balanced();
  {  // move-assignment onto a live handle releases its old value first
    H a, b;
    make(a);
    make(b);
    const auto old = (void*)b.get();
    const auto raw = a.get();
    b = std::move(a);
    CHECK(!a && b.get() == raw && !g.live.count(old) && g.released.back() == old);
  }
  check_balanced();
  {  // self-move keeps the value; reset releases it now; a second reset does nothing
    H a;
    make(a);
    const auto raw = a.get();
    H& same = a;
    a = std::move(same);
    CHECK(a.get() == raw && g.live.count((void*)raw));
    a.reset();
    CHECK(!a && !g.live.count((void*)raw));
    a.reset();
  }
  check_balanced();
  {  // creation on a live handle releases the old value first
    H a;
    make(a);
    const auto old = (void*)a.get();
    make(a);
    CHECK(a && !g.live.count(old));
  }
  check_balanced();
  {  // a failed creation leaves the handle null
    H a;
    g.fail_all = true;
    CHECK(make(a) != hipSuccess && !a);
    g.fail_all = false;
  }
  check_balanced();
}

int main() {
  handle_cases<DeviceBuf<float>>([](DeviceBuf<float>& b) { return b.alloc(10); });
  handle_cases<PinnedBuf<int>>([](PinnedBuf<int>& b) { return b.alloc(11); });
  handle_cases<Event>([](Event& e) { return e.create(); });
  handle_cases<Event>([](Event& e) { return e.create_untimed(); });
  handle_cases<Stream>([](Stream& s) { return s.create(); });
  handle_cases<Stream>([](Stream& s) { return s.create(256); });
  CHECK(g.timed_events > 0 && g.untimed_events > 0 && g.masked_streams > 0 && g.plain_streams > 0);

  {  // sizes: n elements, and a zero-length request allocates one element
    DeviceBuf<double> d;
    PinnedBuf<int> h;
    Arena a;
    int* p = nullptr;
    d.alloc(3);
    CHECK(g.bytes.back() == 3 * sizeof(double));
    d.alloc(0);
    CHECK(g.bytes.back() == sizeof(double) && d);
    h.alloc(0);
    CHECK(g.bytes.back() == sizeof(int) && h);
    CHECK(a.alloc(&p, 0) == hipSuccess && p && g.bytes.back() == sizeof(int));
  }
  check_balanced();

  {  // the masked stream falls back to a plain one, and converts to its raw handle
    g.refuse_masks = true;
    const int plain = g.plain_streams;
    Stream s;
    CHECK(s.create(304) == hipSuccess && s && g.plain_streams == plain + 1);
    hipStream_t raw = s;
    CHECK(raw == s.get());
    g.refuse_masks = false;
  }
  check_balanced();

  {  // an arena releases in reverse order of allocation, once each
    void* order[4];
    const size_t before = g.released.size();
    {
      Arena a;
      float* p[4];
      for (int k = 0; k < 4; k++) {
        CHECK(a.alloc(&p[k], 8 + k) == hipSuccess && g.bytes.back() == (8 + k) * sizeof(float));
        order[k] = p[k];
      }
      CHECK(g.live.size() == 4);
    }
    CHECK(g.released.size() == before + 4);
    for (int k = 0; k < 4; k++) CHECK(g.released[before + k] == order[3 - k]);
  }
  check_balanced();

  {  // a failed n-th allocation in a sequence: the earlier ones stay owned and go at the end of the scope
    const int created = g.created;
    {
      Arena a;
      DeviceBuf<int> x, y, z;
      int *p0 = nullptr, *p1 = nullptr, *p2 = nullptr;
      g.fail_at = 5;
      const bool ok = a.alloc(&p0, 4) == hipSuccess && x.alloc(4) == hipSuccess && a.alloc(&p1, 4) == hipSuccess &&
                      y.alloc(4) == hipSuccess && a.alloc(&p2, 4) == hipSuccess && z.alloc(4) == hipSuccess;
      CHECK(!ok && p0 && p1 && !p2 && x && y && !z);
      CHECK(g.created == created + 4 && g.live.size() == 4);
      g.fail_at = 0;
    }
    CHECK(g.created == created + 4);
  }
  check_balanced();

  {  // handles in a vector (the event pool, a group's states): growth moves them, none is released early or twice
    std::vector<Event> pool;
    for (int k = 0; k < 9; k++) {
      Event e;
      e.create();
      pool.push_back(std::move(e));
    }
    CHECK(g.live.size() == 9);
    Event taken = std::move(pool.back());
    pool.pop_back();
    CHECK(g.live.size() == 9 && taken);
  }
  check_balanced();

  {  // host registrations: unregistered at clear() and at the end of the scope, a refused one not kept
    char a[16], b[16];
    HostRegistrations r;
    CHECK(r.add(a, sizeof a) == hipSuccess && r.add(b, sizeof b) == hipSuccess);
    CHECK(r.add(a, sizeof a) != hipSuccess);
    r.clear();
    CHECK(g.registered.empty());
    r.add(b, sizeof b);
  }
  check_balanced();

  printf("{\"failures\": %d, \"created\": %d, \"released\": %zu}\n", failures, g.created, g.released.size());
  return failures ? 1 : 0;
}
