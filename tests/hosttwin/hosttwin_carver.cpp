// TEST-ONLY host build of the workspace carver (ws_carver.hpp: the arithmetic under ecgpu_carve).  One layout of n sub-buffers
// runs as ecgpu_carve runs it: a sizing pass, then a pointer pass over `base`.  Checked by tests/test_hosttwin_carver.py; with
// -DHOSTTWIN_CARVER_MAIN the file is a program of its own that checks the same properties (for a sanitizer build).
#include <stdint.h>

#include "ws_carver.hpp"

namespace {
struct Wide { uint32_t w[12]; };                    // a 48-byte element, as the P-384 buffers have
// the layout under test: sub-buffer i has sizes[i] bytes; the element types rotate, as they do in a real layout
void layout(WsCarver& ws, const uint64_t* sizes, int n, uint64_t* ptrs) {
  for (int i = 0; i < n; i++) {
    const size_t bytes = (size_t)sizes[i];
    void* p = i % 3 == 0 ? (void*)ws.take<uint8_t>(bytes) : i % 3 == 1 ? (void*)ws.take<uint32_t>(bytes) : (void*)ws.take<Wide>(bytes);
    ptrs[i] = (uint64_t)(uintptr_t)p;
  }
}
}  // namespace

extern "C" {
// base: where the pointer pass carves (an address, never read or written).  size_ptrs / ptrs: the n pointers either pass handed
// out, as integers; totals: the two passes' totals
void ht_carve(uint64_t base, const uint64_t* sizes, int n, uint64_t* size_ptrs, uint64_t* ptrs, uint64_t* totals) {
  WsCarver sizing{nullptr};
  layout(sizing, sizes, n, size_ptrs);
  WsCarver ws{(char*)(uintptr_t)base};
  layout(ws, sizes, n, ptrs);
  totals[0] = sizing.total;
  totals[1] = ws.total;
}
}

#ifdef HOSTTWIN_CARVER_MAIN
#include <stdio.h>
#include <sys/mman.h>
#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)
int main() {
  const uint64_t sizes[] = {0, 1, 255, 256, 257, 0, ((uint64_t)5 << 20) + 3, (uint64_t)3 << 32, 0, 7};
  constexpr int N = sizeof(sizes) / sizeof(sizes[0]);
  uint64_t size_ptrs[N], ptrs[N], totals[2], expect = 0;
  for (uint64_t s : sizes) expect += (s + 255) / 256 * 256;
  // address space only: the pointer pass stays inside one mapping, nothing is touched
  void* base = mmap(nullptr, expect, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  CHECK(base != MAP_FAILED);
  ht_carve((uint64_t)(uintptr_t)base, sizes, N, size_ptrs, ptrs, totals);
  CHECK(totals[0] == expect && totals[1] == expect);
  uint64_t at = (uint64_t)(uintptr_t)base;
  for (int i = 0; i < N; i++) {
    CHECK(size_ptrs[i] == 0);
    CHECK(ptrs[i] == at && (ptrs[i] - (uint64_t)(uintptr_t)base) % 256 == 0);
    at += (sizes[i] + 255) / 256 * 256;
  }
  CHECK(at == (uint64_t)(uintptr_t)base + totals[1]);
  munmap(base, expect);
  printf("carver ok: %d sub-buffers, %llu bytes\n", N, (unsigned long long)totals[1]);
  return 0;
}
#endif
