// TEST-ONLY host build of the k256 multiplications with every operand free: mul(a, b), mul_add2(a, b, e, f) and
// mul_add_sqr(a, b, s) on raw 256-bit inputs (possibly >= p), so that tests/test_hosttwin_k256_fold_first.py can drive
// every column of the schoolbook products to its maximum.  The portable fallback of the column forms drops the carry of
// the products a call site declares carry-free (mac_nc), exactly as the device code does.
#include <string.h>
#include "hosttwin_trace.hpp"
#include "fe_k256.hpp"
using namespace ecgpu;

static void ld_raw(FeK256& f, const uint8_t* b) { u32 w[8]; memcpy(w, b, 32); k256::from_be_words(f, w); }
static void st_raw(uint8_t* b, const FeK256& f) { u32 w[8]; k256::to_be_words(w, f); memcpy(b, w, 32); }

extern "C" {
// op: 0 mul(a, b)   1 mul_add2(a, b, e, f)   2 mul_add_sqr(a, b, e) (f unused)
// The output is the raw, weakly reduced value (not normalised).
int ht_k256_fold_first_op(int op, const uint8_t* a, const uint8_t* b, const uint8_t* e, const uint8_t* f, uint8_t* out, int n) {
  for (int i = 0; i < n; i++) {
    FeK256 x, y, u, v, r;
    ld_raw(x, a + 32 * i); ld_raw(y, b + 32 * i); ld_raw(u, e + 32 * i); ld_raw(v, f + 32 * i);
    switch (op) {
      case 0: k256::mul(r, x, y); break;
      case 1: k256::mul_add2(r, x, y, u, v); break;
      case 2: k256::mul_add_sqr(r, x, y, u); break;
      default: return -1;
    }
    st_raw(out + 32 * i, r);
  }
  return 0;
}
}
