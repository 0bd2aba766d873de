// TEST-ONLY host build of the four k256 products (fe_k256.hpp: mul, sqr, mul_add2, mul_add_sqr and their exact forms) on raw 256-bit
// operands (possibly >= p), with the ECGPU_TAIL_NOTE hook recording, per input, which paths the reduction's tail took: the carries of
// the two chains the overflow count T is assembled on, word 16 of a two-product sum, the carry of the fold's first multiply, the rare
// ripple out of word 2 and the second fold behind it: tests/test_hosttwin_k256_tails.py.
// The product headers are compiled into a namespace of this file's own, because the hook changes the inline functions' bodies and the
// other hosttwin translation units compile them without it.
#include <stdint.h>
#include <string.h>
static uint32_t g_tail_mask, g_tail_bad;
static const char* const TAIL_SITES[7] = {"sqr:c1", "chain:word7", "chain:t0", "mul:h8", "fold:k1", "fold:ripple", "fold:second"};
static void tail_note(const char* site, bool cond) {
  for (int i = 0; i < 7; i++)
    if (strcmp(site, TAIL_SITES[i]) == 0) {
      if (cond) g_tail_mask |= 1u << i;
      return;
    }
  g_tail_bad++;
}
#define ECGPU_TAIL_NOTE(site, cond) tail_note(site, cond)
#define ecgpu ecgpu_tail_twin          // only across the product headers below; every system header is included above
#include "fe_k256.hpp"
#undef ecgpu
using namespace ecgpu_tail_twin;

extern "C" {
// op: 0 mul(a, b)   1 sqr(a)   2 mul_add2(a, b, e, f)   3 mul_add_sqr(a, b, e); exact != 0: the *_exact forms (the same tail behind the
// exact columns).  Operands and results are n x 8 little-endian words; out is the raw, weakly reduced value.  masks[i]: bit k set
// when site k of TAIL_SITES held for input i.  Returns the number of hook calls with an unknown site name (0), -1 for a bad op.
int ht_k256_tail_op(int op, int exact, const uint32_t* a, const uint32_t* b, const uint32_t* e, const uint32_t* f, uint32_t* out,
                    uint32_t* masks, int n) {
  if (op < 0 || op > 3) return -1;
  g_tail_bad = 0;
  for (int i = 0; i < n; i++) {
    FeK256 x, y, u, v, r;
    memcpy(x.v, a + 8 * i, 32); memcpy(y.v, b + 8 * i, 32); memcpy(u.v, e + 8 * i, 32); memcpy(v.v, f + 8 * i, 32);
    g_tail_mask = 0;
    switch (op) {
      case 0: if (exact) k256::mul_exact(r, x, y); else k256::mul(r, x, y); break;
      case 1: if (exact) k256::sqr_exact(r, x); else k256::sqr(r, x); break;
      case 2: if (exact) k256::mul_add2_exact(r, x, y, u, v); else k256::mul_add2(r, x, y, u, v); break;
      case 3: if (exact) k256::mul_add_sqr_exact(r, x, y, u); else k256::mul_add_sqr(r, x, y, u); break;
    }
    memcpy(out + 8 * i, r.v, 32);
    masks[i] = g_tail_mask;
  }
  return (int)g_tail_bad;
}
}
