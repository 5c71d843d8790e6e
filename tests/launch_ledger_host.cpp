// Drives gesture2vec_amd/csrc/launch_ledger.hpp on the CPU with counting stubs in place of the runtime
// (tests/test_launch_ledger_host.py builds and runs it, plain and under ThreadSanitizer).  Exits non-zero at the first failed check.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <set>
#include <thread>
#include <utility>
#include <vector>

#include "launch_ledger.hpp"

using g2v::LaunchLedger;
constexpr size_t LIMIT = g2v::LDS_NO_RESERVE_LIMIT;

#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                      \
    }                                                               \
  } while (0)

static char g_kernels[4];      // four distinct addresses stand for four kernels
static const void* kern(int i) { return &g_kernels[i]; }

// a raise stub that counts its calls and remembers the last request; `ok` is what it answers
struct Raise {
  int calls = 0;
  size_t last = 0;
  bool ok = true;
  bool operator()(const void*, size_t bytes) {
    ++calls;
    last = bytes;
    return ok;
  }
};

static void test_limit() {
  LaunchLedger L;
  Raise r;
  for (size_t b : {(size_t)0, (size_t)1, (size_t)4096, LIMIT - 1, LIMIT}) CHECK(L.reserve(0, kern(0), b, r));
  CHECK(r.calls == 0 && L.granted(0, kern(0)) == 0);
  CHECK(LIMIT == 48 * 1024);
}

static void test_high_water() {
  LaunchLedger L;
  Raise r;
  const size_t up[] = {LIMIT + 16, LIMIT + 1024, LIMIT + 1024, 64 * 1024, 160 * 1024};
  int want = 0;
  size_t mark = 0;
  auto ask = [&](size_t b) {
    if (b > LIMIT && b > mark) { ++want; mark = b; }
    CHECK(L.reserve(0, kern(0), b, r));
    CHECK(r.calls == want && L.granted(0, kern(0)) == mark);
    if (b == mark && want) CHECK(r.last == mark);
  };
  for (size_t b : up) ask(b);                                   // ascending: one call per new strict maximum
  for (int i = 4; i >= 0; --i) ask(up[i]);                      // descending: none
  for (int k = 0; k < 3; ++k) ask(160 * 1024);                  // repeated: none
  ask(1024);
  ask(160 * 1024 + 4);                                          // a new maximum after all that
  CHECK(want == 5);
}

static void test_refusal_not_remembered() {
  LaunchLedger L;
  Raise r;
  r.ok = false;
  CHECK(!L.reserve(0, kern(0), 80 * 1024, r) && r.calls == 1 && L.granted(0, kern(0)) == 0);
  CHECK(!L.reserve(0, kern(0), 80 * 1024, r) && r.calls == 2);      // the same request asks again
  r.ok = true;
  CHECK(L.reserve(0, kern(0), 80 * 1024, r) && r.calls == 3 && L.granted(0, kern(0)) == 80 * 1024);
  CHECK(L.reserve(0, kern(0), 80 * 1024, r) && r.calls == 3);       // granted: asked no more
  r.ok = false;                                                     // a later refusal leaves the earlier grant in place
  CHECK(!L.reserve(0, kern(0), 96 * 1024, r) && r.calls == 4 && L.granted(0, kern(0)) == 80 * 1024);
  CHECK(L.reserve(0, kern(0), 72 * 1024, r) && r.calls == 4);
}

static void test_independent_keys() {
  LaunchLedger L;
  Raise r;
  int want = 0;
  for (int dev = 0; dev < 2; ++dev)
    for (int k = 0; k < 2; ++k) {
      CHECK(L.reserve(dev, kern(k), 100 * 1024, r) && r.calls == ++want);      // a grant to one (device, kernel) is no grant to another
      CHECK(L.reserve(dev, kern(k), 100 * 1024, r) && r.calls == want);
    }
  CHECK(L.reserve(1, kern(1), 120 * 1024, r) && r.calls == ++want);
  CHECK(L.granted(0, kern(0)) == 100 * 1024 && L.granted(0, kern(1)) == 100 * 1024 && L.granted(1, kern(0)) == 100 * 1024 &&
        L.granted(1, kern(1)) == 120 * 1024);
}

static void test_resident() {
  LaunchLedger L;
  Raise r;
  int asks = 0, raises_at_ask = -1;
  bool answer = true;
  auto ask = [&](const void*, int, size_t) {
    ++asks;
    raises_at_ask = r.calls;
    return answer;
  };
  CHECK(L.resident(0, kern(0), 256, 100 * 1024, r, ask) && asks == 1 && r.calls == 1);
  CHECK(raises_at_ask == 1);                                                            // it reserved before it asked
  CHECK(L.resident(0, kern(0), 256, 100 * 1024, r, ask) && asks == 1 && r.calls == 1);  // a positive answer is remembered
  answer = false;
  CHECK(!L.resident(0, kern(0), 192, 100 * 1024, r, ask) && asks == 2);                 // keyed by block ...
  CHECK(!L.resident(0, kern(0), 192, 100 * 1024, r, ask) && asks == 2);                 // ... and a negative answer is remembered too
  CHECK(!L.resident(0, kern(0), 256, 0, r, ask) && asks == 3 && r.calls == 1);          // keyed by bytes; nothing to reserve at 0
  CHECK(!L.resident(0, kern(0), 256, 0, r, ask) && asks == 3);
  answer = true;
  CHECK(L.resident(1, kern(0), 256, 0, r, ask) && asks == 4);                           // another device, another kernel: asked anew
  CHECK(L.resident(0, kern(1), 256, 0, r, ask) && asks == 5);
  CHECK(L.resident(0, kern(0), 256, 100 * 1024, r, ask) && asks == 5);
  r.ok = false;                                                                         // a refused reservation: "no", nothing asked or kept
  CHECK(!L.resident(0, kern(2), 256, 100 * 1024, r, ask) && asks == 5 && r.calls == 2);
  r.ok = true;
  CHECK(L.resident(0, kern(2), 256, 100 * 1024, r, ask) && asks == 6 && r.calls == 3);
}

static void test_cus() {
  LaunchLedger L;
  int asks = 0;
  auto ask = [&](int dev) {
    ++asks;
    return 256 - dev;
  };
  CHECK(L.cus(0, ask) == 256 && L.cus(0, ask) == 256 && asks == 1);
  CHECK(L.cus(1, ask) == 255 && L.cus(1, ask) == 255 && L.cus(0, ask) == 256 && asks == 2);
}

// eight threads, mixed requests over 4 kernels x 2 devices.  The stubs' counters are plain variables: the ledger promises that a
// callable runs under its mutex, and ThreadSanitizer reports it if one does not.
static void test_threads() {
  constexpr int NTHREAD = 8, NREQ = 4000, NK = 4, NDEV = 2;
  const size_t sizes[] = {1024, LIMIT, LIMIT + 64, 56 * 1024, 64 * 1024, 96 * 1024, 128 * 1024, 160 * 1024};
  constexpr int NS = sizeof(sizes) / sizeof(sizes[0]);
  LaunchLedger L;
  int raises[NDEV][NK] = {};
  int asks = 0, cu_asks = 0;
  size_t largest[NTHREAD][NDEV][NK] = {};
  std::vector<std::thread> th;
  for (int t = 0; t < NTHREAD; ++t)
    th.emplace_back([&, t] {
      unsigned s = 12345u + 977u * t;
      for (int i = 0; i < NREQ; ++i) {
        s = s * 1664525u + 1013904223u;
        const int dev = (s >> 8) % NDEV, k = (s >> 12) % NK;
        // thread t starts low and reaches the top sizes only late: the marks keep rising while others ask for less
        const size_t b = sizes[(s >> 16) % (1 + std::min(NS - 1, (i * NS) / NREQ + (t & 1)))];
        auto raise = [&](const void*, size_t) {
          ++raises[dev][k];
          return true;
        };
        bool ok;
        if ((s >> 28) & 1)
          ok = L.resident(dev, kern(k), 256, b, raise, [&](const void*, int, size_t) { ++asks; return true; });
        else
          ok = L.reserve(dev, kern(k), b, raise);
        if (!ok) { fprintf(stderr, "a request was refused\n"); exit(1); }
        if ((s >> 29) & 1) (void)L.cus(dev, [&](int) { ++cu_asks; return 256; });
        largest[t][dev][k] = std::max(largest[t][dev][k], b);
      }
    });
  for (auto& x : th) x.join();
  int above = 0;
  for (size_t b : sizes) above += b > LIMIT;
  for (int dev = 0; dev < NDEV; ++dev)
    for (int k = 0; k < NK; ++k) {
      size_t top = 0;
      for (int t = 0; t < NTHREAD; ++t) top = std::max(top, largest[t][dev][k]);
      CHECK(top == 160 * 1024);                                      // (the run did reach the top size on every key)
      CHECK(L.granted(dev, kern(k)) == top);
      CHECK(raises[dev][k] >= 1 && raises[dev][k] <= above);
    }
  CHECK(asks >= 1 && asks <= NDEV * NK * NS && cu_asks == NDEV);
}

int main() {
  test_limit();
  test_high_water();
  test_refusal_not_remembered();
  test_independent_keys();
  test_resident();
  test_cus();
  test_threads();
  printf("launch ledger ok\n");
  return 0;
}
