// ggs_host_debug.hpp -- what the ggs_debug_* entry points (the primitives of the parity tests) share: the device memory of one call.
#pragma once
#include "ggs_host_state.hpp"

namespace {
struct TmpDev {
  std::vector<void *> p;
  ~TmpDev() { for (void *q : p) if (q) (void)hipFree(q); }
  void *get(size_t bytes) { void *q = nullptr; if (hipMalloc(&q, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr; p.push_back(q); return q; }
};
}  // namespace
