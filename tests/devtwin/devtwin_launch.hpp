// TEST-ONLY host-side plumbing shared by the launchers of devtwin_group.hip and devtwin_rfc6979.hip: device copies of host word
// arrays that free themselves, and the first-error return of an entry point.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "mp32.hpp"

namespace ecgpu {
namespace twin {

// device copies of up to MAXN host arrays; the destructor frees whatever was allocated
struct DevArrays {
  static constexpr int MAXN = 6;
  void* p[MAXN] = {};
  int count = 0;
  ~DevArrays() {
    for (int k = 0; k < count; k++) (void)hipFree(p[k]);
  }
  hipError_t in(const u32*& d, const u32* h, size_t words) {
    if (count >= MAXN) return hipErrorInvalidValue;
    void* q = nullptr;
    hipError_t err = hipMalloc(&q, words * sizeof(u32));
    if (err != hipSuccess) return err;
    p[count++] = q;
    d = static_cast<const u32*>(q);
    return hipMemcpy(q, h, words * sizeof(u32), hipMemcpyHostToDevice);
  }
  hipError_t outbuf(u32*& d, size_t words) {
    if (count >= MAXN) return hipErrorInvalidValue;
    void* q = nullptr;
    hipError_t err = hipMalloc(&q, words * sizeof(u32));
    if (err != hipSuccess) return err;
    p[count++] = q;
    d = static_cast<u32*>(q);
    return hipMemset(q, 0, words * sizeof(u32));
  }
};

#define DT_CHECK(x)                          \
  do {                                       \
    hipError_t err_ = (x);                   \
    if (err_ != hipSuccess) return (int)err_; \
  } while (0)

}  // namespace twin
}  // namespace ecgpu
