// TEST-ONLY host-side plumbing shared by the launchers of devtwin_group.hip, devtwin_rfc6979.hip and devtwin_ecdsa.hip: device
// copies of host word arrays that free themselves, and the first-error return of an entry point.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "mp32.hpp"

namespace ecgpu {
namespace twin {

// device copies of up to MAXN host arrays; the destructor frees whatever was allocated
struct DevArrays {
  static constexpr int MAXN = 8;
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
  // the same for byte arrays (flags, one per row), held in whole words on the device
  hipError_t in_bytes(const uint8_t*& d, const uint8_t* h, size_t bytes) {
    u32* q = nullptr;
    hipError_t err = outbuf(q, (bytes + 3) / 4);
    if (err != hipSuccess) return err;
    d = reinterpret_cast<const uint8_t*>(q);
    return hipMemcpy(q, h, bytes, hipMemcpyHostToDevice);
  }
  hipError_t outbuf_bytes(uint8_t*& d, size_t bytes) {
    u32* q = nullptr;
    hipError_t err = outbuf(q, (bytes + 3) / 4);
    d = reinterpret_cast<uint8_t*>(q);
    return err;
  }
};

#define DT_CHECK(x)                          \
  do {                                       \
    hipError_t err_ = (x);                   \
    if (err_ != hipSuccess) return (int)err_; \
  } while (0)

}  // namespace twin
}  // namespace ecgpu
