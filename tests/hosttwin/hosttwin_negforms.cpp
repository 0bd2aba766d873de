// TEST-ONLY host build of the sign-tracking forms of the k256 throughput loop (fe_k256.hpp: half, sub2, mul_add_sqr;
// mulfast_k256.hpp: jac_double_neg, jac_add_mixed_neg).  Checked by tests/test_hosttwin_k256_neg_forms.py.
#include <string.h>
#include "hosttwin_trace.hpp"
#include "mul_k256.hpp"
#include "mulfast_k256.hpp"
using namespace ecgpu;

static void ld(FeK256& f, const uint8_t* b) { u32 w[8]; memcpy(w, b, 32); k256::from_be_words(f, w); }
static void st_raw(uint8_t* b, const FeK256& f) { u32 w[8]; k256::to_be_words(w, f); memcpy(b, w, 32); }
static void st(uint8_t* b, const FeK256& f0) { FeK256 f; k256::normalize(f, f0); st_raw(b, f); }

extern "C" {
// op: 0 half(x)   1 sub2(x, y, ~y)   2 mul_add_sqr(x, y, y) = xy + y^2   3 mul_add_sqr(~x, ~y, ~x) (up to 2^513)
// Inputs are raw 256-bit integers (possibly >= p); the output is the raw, weakly reduced value (not normalised).
int ht_k256_negforms_fe_op(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, int n) {
  for (int i = 0; i < n; i++) {
    FeK256 x, y, r, cx, cy;
    ld(x, a + 32 * i); ld(y, b + 32 * i);
    for (int w = 0; w < 8; w++) { cx.v[w] = ~x.v[w]; cy.v[w] = ~y.v[w]; }
    switch (op) {
      case 0: k256::half(r, x); break;
      case 1: k256::sub2(r, x, y, cy); break;
      case 2: k256::mul_add_sqr(r, x, y, y); break;
      case 3: k256::mul_add_sqr(r, cx, cy, cx); break;
      default: return -1;
    }
    st_raw(out + 32 * i, r);
  }
  return 0;
}
// out = -(P + Q) (P Jacobian X||Y||Z, Q affine x||y) and -2P, Jacobian X||Y||Z (canonical bytes)
int ht_k256_jac_add_mixed_neg(const uint8_t* p, const uint8_t* q, uint8_t* out, int n) {
  for (int i = 0; i < n; i++) {
    JacK256 a; ld(a.x, p + 96 * i); ld(a.y, p + 96 * i + 32); ld(a.z, p + 96 * i + 64);
    FeK256 x, y; ld(x, q + 64 * i); ld(y, q + 64 * i + 32);
    k256::jac_add_mixed_neg(a, x, y);
    st(out + 96 * i, a.x); st(out + 96 * i + 32, a.y); st(out + 96 * i + 64, a.z);
  }
  return 0;
}
int ht_k256_jac_double_neg(const uint8_t* p, uint8_t* out, int n) {
  for (int i = 0; i < n; i++) {
    JacK256 a; ld(a.x, p + 96 * i); ld(a.y, p + 96 * i + 32); ld(a.z, p + 96 * i + 64);
    k256::jac_double_neg(a);
    st(out + 96 * i, a.x); st(out + 96 * i + 32, a.y); st(out + 96 * i + 64, a.z);
  }
  return 0;
}
}
