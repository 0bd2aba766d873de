// What every message of one expand_message_xmd call shares (h2c_hash.hpp has the kernels): plain data, filled on the host by the
// entry points (ecgpu.hip) and passed to the kernels BY VALUE - kernel-argument memory, so the DST costs no copy and no allocation.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ecgpu {
namespace h2c {

// bytes = I2OSP(len_in_bytes, 2) || I2OSP(0, 1) || DST || I2OSP(len(DST), 1): b_0 takes all of it, the later blocks skip the first 3
struct XmdTail {
  uint8_t bytes[3 + 255 + 1];
  uint32_t len;                  // 3 + len(DST) + 1
  uint32_t out_len;              // len_in_bytes
};
// dst_len in 1 .. 255, out_len below 2^16 (the callers check)
static inline void xmd_tail_set(XmdTail& t, const uint8_t* dst, size_t dst_len, size_t out_len) {
  t.bytes[0] = (uint8_t)(out_len >> 8);
  t.bytes[1] = (uint8_t)out_len;
  t.bytes[2] = 0;
  for (size_t i = 0; i < 256; i++) t.bytes[3 + i] = i < dst_len ? dst[i] : 0;
  t.bytes[3 + dst_len] = (uint8_t)dst_len;
  t.len = (uint32_t)(3 + dst_len + 1);
  t.out_len = (uint32_t)out_len;
}

}  // namespace h2c
}  // namespace ecgpu
