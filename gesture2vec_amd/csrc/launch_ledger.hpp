// launch_ledger.hpp -- what a launch needs settled before it goes out, remembered per device: how much dynamic LDS each kernel has
// been granted, whether one workgroup of a persistent kernel fits a CU, and the CU count.  Plain C++17 (no HIP include): the
// runtime calls come in as callables, so a CPU program can drive the bookkeeping (tests/test_launch_ledger_host.py).  misc.hip owns
// the one instance and supplies the runtime (g2v_internal_lds_reserve, g2v_internal_kernel_resident, g2v_internal_device_cus).
// The facts belong to a code object on a device and neither changes inside a process; every access, the callable included, runs
// under one mutex.
#pragma once
#include <stddef.h>

#include <map>
#include <mutex>
#include <tuple>
#include <utility>

namespace g2v {

// dynamic LDS a kernel gets without asking for it; above it a launch has to be preceded by a granted reservation
constexpr size_t LDS_NO_RESERVE_LIMIT = 48 * 1024;

class LaunchLedger {
 public:
  // May `fn` be launched on `dev` with `bytes` of dynamic LDS?  `raise(fn, bytes)` -> bool is called only for a request above the
  // limit AND above what (dev, fn) has been granted; a refusal records nothing, so the same request asks again.
  template <class Raise>
  bool reserve(int dev, const void* fn, size_t bytes, Raise&& raise) {
    std::lock_guard<std::mutex> lock(mu_);
    return reserve_locked(dev, fn, bytes, raise);
  }
  // Does at least one workgroup of `block` threads and `bytes` of dynamic LDS fit a CU?  Reserves as above, then asks
  // `ask(fn, block, bytes)` -> bool once per (dev, fn, block, bytes) and remembers the answer, yes or no.  (A refused
  // reservation answers no and is, as above, not remembered.)
  template <class Raise, class Ask>
  bool resident(int dev, const void* fn, int block, size_t bytes, Raise&& raise, Ask&& ask) {
    std::lock_guard<std::mutex> lock(mu_);
    if (!reserve_locked(dev, fn, bytes, raise)) return false;
    const auto key = std::make_tuple(dev, fn, block, bytes);
    auto it = resident_.find(key);
    if (it == resident_.end()) it = resident_.emplace(key, (bool)ask(fn, block, bytes)).first;
    return it->second;
  }
  // CU count of `dev`: `ask(dev)` -> int once per device
  template <class Ask>
  int cus(int dev, Ask&& ask) {
    std::lock_guard<std::mutex> lock(mu_);
    auto it = cus_.find(dev);
    if (it == cus_.end()) it = cus_.emplace(dev, (int)ask(dev)).first;
    return it->second;
  }
  // what (dev, fn) has been granted so far (0: nothing asked for, or nothing above the limit)
  size_t granted(int dev, const void* fn) {
    std::lock_guard<std::mutex> lock(mu_);
    const auto it = lds_.find(std::make_pair(dev, fn));
    return it == lds_.end() ? 0 : it->second;
  }

 private:
  template <class Raise>
  bool reserve_locked(int dev, const void* fn, size_t bytes, Raise& raise) {
    if (bytes <= LDS_NO_RESERVE_LIMIT) return true;
    const auto key = std::make_pair(dev, fn);
    const auto it = lds_.find(key);
    if (it != lds_.end() && bytes <= it->second) return true;
    if (!raise(fn, bytes)) return false;
    lds_[key] = bytes;
    return true;
  }
  std::mutex mu_;
  std::map<std::pair<int, const void*>, size_t> lds_;
  std::map<std::tuple<int, const void*, int, size_t>, bool> resident_;
  std::map<int, int> cus_;
};

}  // namespace g2v
