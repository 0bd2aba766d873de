// Carves one buffer into sub-buffers of 256-byte-aligned sizes: the arithmetic only, no HIP, so that the host twin tests it.
// A layout asks for its sub-buffers with take<T>(bytes), in order, and runs twice (ecgpu_carve, ecgpu_internal.hpp): on a carver
// without a base to add the sizes up, then, the buffer reserved, on one over the buffer to receive the pointers.
#pragma once
#include <stddef.h>

struct WsCarver {
  char* base;             // nullptr: the sizing pass, every take returns nullptr
  size_t total = 0;       // bytes handed out so far: the offset of the next sub-buffer
  template <class T>
  T* take(size_t bytes) {
    T* p = base ? (T*)(base + total) : nullptr;
    total += (bytes + 255) & ~(size_t)255;
    return p;
  }
};
