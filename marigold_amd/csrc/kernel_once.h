// "Once per kernel": the bookkeeping behind mg_kernel_max_lds (common.h; runtime.hip instantiates it with HIP's attribute call).
// No HIP in here, so a host program can drive it with a setter of its own (tests/host_cpp/kernel_once_main.cpp).
#pragma once
#include <mutex>
#include <unordered_map>

// The largest size `set` has succeeded with, per kernel address.  raise() is safe from any number of host threads making the first
// launch of the same or of different kernels at once: the table and the call of `set` are under one mutex, so a kernel is set at
// most once per size and a launch never runs ahead of its kernel's attribute.
class mg_kernel_once {
 public:
  // -> 0 once `kern` is set to `bytes` or more; else what `set(kern, bytes)` returned (non-zero: nothing is recorded and the next
  // call tries again).  `dry`: nothing is set, nothing is recorded.
  template <class Set>
  int raise(const void* kern, int bytes, bool dry, Set&& set) {
    if (dry) return 0;
    std::lock_guard<std::mutex> lk(mutex_);
    const auto it = set_bytes_.find(kern);
    if (it != set_bytes_.end() && it->second >= bytes) return 0;
    if (const int rc = set(kern, bytes)) return rc;
    set_bytes_[kern] = bytes;
    return 0;
  }

 private:
  std::mutex mutex_;
  std::unordered_map<const void*, int> set_bytes_;
};
