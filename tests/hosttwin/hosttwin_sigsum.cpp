// TEST-ONLY host build of csrc/affine_ops.hpp over arrays: the affine sum with flags (the batched driver in the kernels' lane
// layout, and sum_kind + slope_terms one pair at a time), y from x, the canonical and curve checks.  The ECGPU_EXC_NOTE counters
// (ht_exc_reset / ht_exc_counts) say which arm each pair entered.  Checked against the oracle by tests/test_hosttwin_sigsum.py.
#include "hosttwin_trace.hpp"
#include <string.h>
#include <vector>
#include "affine_ops.hpp"
using namespace ecgpu;

namespace {
std::vector<u32> words(const uint8_t* p, size_t bytes) {
  std::vector<u32> w(bytes / 4 + 1);
  memcpy(w.data(), p, bytes);
  return w;
}

// A + B of n pairs as a launch of T lanes walks them: lane l takes l, l + T, .. in batches of 16 (the product's batch)
template <class C>
void sum_batch(const uint8_t* a_xy, const uint8_t* a_inf, const uint8_t* b_xy, const uint8_t* b_inf, const uint8_t* ok, size_t n, size_t T, uint8_t* out_xy,
               uint8_t* kinds) {
  constexpr int L = C::NW, BATCH = 16;
  const std::vector<u32> a = words(a_xy, n * 8 * L), b = words(b_xy, n * 8 * L);
  std::vector<u32> out(n * 2 * L);
  for (size_t tid = 0; tid < T; tid++)
    for (size_t base = tid; base < n; base += T * BATCH)
      aff::sum_batch<C, BATCH>(a.data(), a_inf, b.data(), b_inf, ok, base, T, n, [&](size_t i, u32 kind, const typename C::Fe& x3, const typename C::Fe& y3) {
        C::fe_store(&out[i * 2 * L], x3);
        C::fe_store(&out[i * 2 * L + L], y3);
        kinds[i] = (uint8_t)kind;
      });
  memcpy(out_xy, out.data(), n * 8 * L);
}

// the same sums from sum_kind and slope_terms alone, one inversion per pair
template <class C>
void sum_each(const uint8_t* a_xy, const uint8_t* a_inf, const uint8_t* b_xy, const uint8_t* b_inf, size_t n, uint8_t* out_xy, uint8_t* kinds) {
  using Fe = typename C::Fe;
  constexpr int L = C::NW;
  const std::vector<u32> a = words(a_xy, n * 8 * L), b = words(b_xy, n * 8 * L);
  std::vector<u32> out(n * 2 * L);
  for (size_t i = 0; i < n; i++) {
    const u32 *pa = &a[i * 2 * L], *pb = &b[i * 2 * L];
    const u32 kind = aff::sum_kind<C>(pa, a_inf[i] != 0, pb, b_inf[i] != 0);
    Fe x3, y3;
    C::fe_zero(x3); C::fe_zero(y3);
    if (kind == aff::SUM_OPERAND) {
      C::fe_load(x3, a_inf[i] ? pb : pa);
      C::fe_load(y3, (a_inf[i] ? pb : pa) + L);
    } else if (kind & aff::SUM_CHORD) {
      Fe xa, ya, xb, yb, N, D, lam, t;
      C::fe_load(xa, pa); C::fe_load(ya, pa + L);
      C::fe_load(xb, pb); C::fe_load(yb, pb + L);
      aff::slope_terms<C>(N, D, xa, ya, xb, yb, kind == aff::SUM_TANGENT);
      C::fe_inv(D, D);
      C::fe_mul(lam, N, D);
      C::fe_sqr(x3, lam);
      C::fe_sub(x3, x3, xa); C::fe_sub(x3, x3, xb);
      C::fe_sub(t, xa, x3);
      C::fe_mul(y3, lam, t);
      C::fe_sub(y3, y3, ya);
    }
    C::fe_store(&out[i * 2 * L], x3);
    C::fe_store(&out[i * 2 * L + L], y3);
    kinds[i] = (uint8_t)kind;
  }
  memcpy(out_xy, out.data(), n * 8 * L);
}

// per x: canonical, sqrt_rhs (has, y, -y) and lift_x at the wanted parity
template <class C>
void lift(const uint8_t* xs, const uint8_t* odd, size_t n, uint8_t* canon, uint8_t* has, uint8_t* roots, uint8_t* lifted) {
  using Fe = typename C::Fe;
  constexpr int L = C::NW;
  const std::vector<u32> x = words(xs, n * 4 * L);
  std::vector<u32> r(n * 2 * L), l(n * L);
  for (size_t i = 0; i < n; i++) {
    Fe fx, y, ny, yl;
    canon[i] = aff::coords_canonical<C>(&x[i * L]) ? 1 : 0;
    C::fe_load(fx, &x[i * L]);
    const bool h = aff::sqrt_rhs<C>(y, ny, fx);
    const bool h2 = aff::lift_x<C>(yl, fx, odd[i] != 0);
    has[i] = (uint8_t)((h ? 1 : 0) | (h2 ? 2 : 0));
    C::fe_store(&r[i * 2 * L], y);
    C::fe_store(&r[i * 2 * L + L], ny);
    C::fe_store(&l[i * L], yl);
  }
  memcpy(roots, r.data(), n * 8 * L);
  memcpy(lifted, l.data(), n * 4 * L);
}

template <class C>
void curve_check(const uint8_t* xy, size_t n, uint8_t* canon, uint8_t* on) {
  constexpr int L = C::NW;
  const std::vector<u32> p = words(xy, n * 8 * L);
  for (size_t i = 0; i < n; i++) {
    typename C::Fe x, y;
    canon[i] = aff::coords_canonical<C>(&p[i * 2 * L], &p[i * 2 * L + L]) ? 1 : 0;
    C::fe_load(x, &p[i * 2 * L]);
    C::fe_load(y, &p[i * 2 * L + L]);
    on[i] = aff::on_curve<C>(x, y) ? 1 : 0;
  }
}
}  // namespace

extern "C" {
int ht_aff_sum_batch(int curve, const uint8_t* a_xy, const uint8_t* a_inf, const uint8_t* b_xy, const uint8_t* b_inf, const uint8_t* ok, size_t n, size_t T,
                     uint8_t* out_xy, uint8_t* kinds) {
#define ARGS (a_xy, a_inf, b_xy, b_inf, ok, n, T, out_xy, kinds)
  switch (curve) {
    case 0: sum_batch<CurveK256> ARGS; return 0;
    case 1: sum_batch<CurveP256> ARGS; return 0;
    case 2: sum_batch<CurveP384> ARGS; return 0;
  }
#undef ARGS
  return -1;
}
int ht_aff_sum_each(int curve, const uint8_t* a_xy, const uint8_t* a_inf, const uint8_t* b_xy, const uint8_t* b_inf, size_t n, uint8_t* out_xy, uint8_t* kinds) {
#define ARGS (a_xy, a_inf, b_xy, b_inf, n, out_xy, kinds)
  switch (curve) {
    case 0: sum_each<CurveK256> ARGS; return 0;
    case 1: sum_each<CurveP256> ARGS; return 0;
    case 2: sum_each<CurveP384> ARGS; return 0;
  }
#undef ARGS
  return -1;
}
int ht_aff_lift(int curve, const uint8_t* xs, const uint8_t* odd, size_t n, uint8_t* canon, uint8_t* has, uint8_t* roots, uint8_t* lifted) {
#define ARGS (xs, odd, n, canon, has, roots, lifted)
  switch (curve) {
    case 0: lift<CurveK256> ARGS; return 0;
    case 1: lift<CurveP256> ARGS; return 0;
    case 2: lift<CurveP384> ARGS; return 0;
  }
#undef ARGS
  return -1;
}
int ht_aff_curve_check(int curve, const uint8_t* xy, size_t n, uint8_t* canon, uint8_t* on) {
#define ARGS (xy, n, canon, on)
  switch (curve) {
    case 0: curve_check<CurveK256> ARGS; return 0;
    case 1: curve_check<CurveP256> ARGS; return 0;
    case 2: curve_check<CurveP384> ARGS; return 0;
  }
#undef ARGS
  return -1;
}
}
