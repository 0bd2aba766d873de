// TEST-ONLY: records which precomputed-table entries the device templates read (ECGPU_TABLE_TOUCH hook, mp32.hpp) and counts
// the exceptional cases the point additions meet (ECGPU_EXC_NOTE hook, mp32.hpp; ht_exc_reset / ht_exc_counts read them).
// Included before the product headers by every hosttwin translation unit.
#pragma once
#include <stddef.h>
extern "C" void ht_trace_push(int idx);
#define ECGPU_TABLE_TOUCH(idx) ht_trace_push((int)(idx))
extern "C" void ht_exc_push(const char* site);
#define ECGPU_EXC_NOTE(site, cond) do { if (cond) ht_exc_push(site); } while (0)
