// TEST-ONLY host build of the shared-point bodies (csrc/sharedbase.hpp): the two builder stages walked entry run by entry run, and
// mul_shared_one walked element by element over tables built that way, on either accumulator the kernels use (XYZZ: the 256-bit
// curves; Jacobian: P-384).  The ECGPU_EXC_NOTE counters (ht_exc_reset / ht_exc_counts) say which exceptional branches of the
// additions the related points entered.  Checked against the oracle by tests/test_hosttwin_shared.py.
#include "hosttwin_trace.hpp"
#include <string.h>
#include <vector>
#include "traits.hpp"
#include "msm.hpp"
#include "sharedbase.hpp"
using namespace ecgpu;

template <class C> static void load(typename C::Fe& f, const uint8_t* b) { u32 w[C::NW]; memcpy(w, b, C::NB); C::fe_load(f, w); }
template <class C> static void store(uint8_t* b, const typename C::Fe& f) { u32 w[C::NW]; C::fe_store(w, f); memcpy(b, w, C::NB); }

// the table of `point` (canonical x || y) as the device builds it: stage A per window, stage B per run of SHARED_RUN entries
template <class C, int WB>
static void build(std::vector<AffEntry<C>>& table, const uint8_t* point) {
  constexpr int NWIN = fb::nwin_wide<C, WB>(), ENTRIES = fb::wide_entries<WB>();
  AffEntry<C> h;
  load<C>(h.x, point);
  load<C>(h.y, point + C::NB);
  table.resize((size_t)NWIN * ENTRIES);
  for (int j = 0; j < NWIN; j++) {
    AffEntry<C> b;
    fb::shared_window_base<C>(b, h, WB * j);
    for (int q = 0; q < ENTRIES / fb::SHARED_RUN; q++) fb::shared_run<C>(&table[(size_t)j * ENTRIES + q * fb::SHARED_RUN], b, (u32)(q * fb::SHARED_RUN) + 1u);
  }
}
template <class C, int WB>
static int table_out(const uint8_t* point, uint8_t* out_xy) {
  std::vector<AffEntry<C>> t;
  build<C, WB>(t, point);
  for (size_t e = 0; e < t.size(); e++) { store<C>(out_xy + 2 * C::NB * e, t[e].x); store<C>(out_xy + 2 * C::NB * e + C::NB, t[e].y); }
  return (int)t.size();
}

// the two accumulators of fixedbase.hpp's FbAcc, without its device-only epilogue
template <class C>
struct XyzzAcc {
  using Pt = msm::Xyzz<C>;
  static void set_infinity(Pt& p) { msm::xyzz_set_infinity<C>(p); }
  static void add_mixed(Pt& p, const typename C::Fe& x, const typename C::Fe& y) { msm::xyzz_add_mixed<C>(p, x, y); }
  static void add_affine(Pt& p, const typename C::Fe& x, const typename C::Fe& y) { msm::xyzz_add_affine<C>(p, x, y); }
  static bool affine(typename C::Fe& x, typename C::Fe& y, const Pt& p) {
    if (C::fe_is_zero(p.zz)) return false;
    typename C::Fe i;
    C::fe_inv(i, p.zz); C::fe_mul(x, p.x, i);
    C::fe_inv(i, p.zzz); C::fe_mul(y, p.y, i);
    return true;
  }
};
template <class C>
struct JacAcc {
  using Pt = Jac<C>;
  static void set_infinity(Pt& p) { jac::set_infinity<C>(p); }
  static void add_mixed(Pt& p, const typename C::Fe& x, const typename C::Fe& y) { jac::add_mixed<C>(p, x, y); }
  static void add_affine(Pt& p, const typename C::Fe& x, const typename C::Fe& y) { jac::add_affine<C>(p, x, y); }
  static bool affine(typename C::Fe& x, typename C::Fe& y, const Pt& p) {
    if (C::fe_is_zero(p.z)) return false;
    typename C::Fe i, t;
    C::fe_inv(i, p.z); C::fe_sqr(t, i); C::fe_mul(x, p.x, t);
    C::fe_mul(t, t, i); C::fe_mul(y, p.y, t);
    return true;
  }
};

// out[i] = sum_t scalars[i terms + t] points[t]; an all-zero point is the identity (no table)
template <class C, int WB, class Acc>
static int mul(const uint8_t* points, int terms, const uint8_t* scalars, uint8_t* out_xy, uint8_t* out_inf, int n) {
  if (terms < 1 || terms > fb::SHARED_MAX_TERMS) return -1;
  std::vector<AffEntry<C>> tables[fb::SHARED_MAX_TERMS];
  fb::SharedTabs<C> tabs;
  tabs.terms = terms;
  for (int t = 0; t < fb::SHARED_MAX_TERMS; t++) {
    tabs.t[t] = nullptr;
    if (t >= terms) continue;
    const uint8_t* p = points + 2 * C::NB * t;
    uint8_t z = 0;
    for (int b = 0; b < 2 * C::NB; b++) z |= p[b];
    if (!z) continue;
    build<C, WB>(tables[t], p);
    tabs.t[t] = tables[t].data();
  }
  std::vector<u32> sc((size_t)terms * C::NW);
  for (int i = 0; i < n; i++) {
    memcpy(sc.data(), scalars + (size_t)i * terms * C::NB, (size_t)terms * C::NB);
    typename Acc::Pt acc;
    fb::mul_shared_one<C, WB, Acc>(acc, sc.data(), tabs);
    typename C::Fe x, y;
    const bool finite = Acc::affine(x, y, acc);
    if (!finite) { C::fe_zero(x); C::fe_zero(y); }
    store<C>(out_xy + 2 * C::NB * i, x);
    store<C>(out_xy + 2 * C::NB * i + C::NB, y);
    out_inf[i] = finite ? 0 : 1;
  }
  return 0;
}
template <class C, int WB>
static int mul_acc(int jacobian, const uint8_t* points, int terms, const uint8_t* scalars, uint8_t* out_xy, uint8_t* out_inf, int n) {
  return jacobian ? mul<C, WB, JacAcc<C>>(points, terms, scalars, out_xy, out_inf, n) : mul<C, WB, XyzzAcc<C>>(points, terms, scalars, out_xy, out_inf, n);
}

extern "C" {
// entries of the table, or -1; out_xy: nwin_wide x wide_entries rows of canonical x || y.  wb: 5 | 8
int ht_shared_table(int curve, int wb, const uint8_t* point, uint8_t* out_xy) {
#define HT_TABLE(C) (wb == 5 ? table_out<C, 5>(point, out_xy) : wb == 8 ? table_out<C, 8>(point, out_xy) : -1)
  return curve == 0 ? HT_TABLE(CurveK256) : curve == 1 ? HT_TABLE(CurveP256) : curve == 2 ? HT_TABLE(CurveP384) : -1;
#undef HT_TABLE
}
int ht_shared_windows(int curve, int wb) {
  if (wb != 5 && wb != 8) return -1;
  if (curve == 2) return wb == 5 ? fb::nwin_wide<CurveP384, 5>() : fb::nwin_wide<CurveP384, 8>();
  return wb == 5 ? fb::nwin_wide<CurveK256, 5>() : fb::nwin_wide<CurveK256, 8>();
}
// mul_shared_one over `terms` points (canonical x || y rows, zeros = the identity); jacobian: 0 = the XYZZ accumulator, 1 = the Jacobian one
int ht_shared_mul(int curve, int wb, int jacobian, const uint8_t* points, int terms, const uint8_t* scalars, uint8_t* out_xy, uint8_t* out_inf, int n) {
#define HT_MUL(C) (wb == 5 ? mul_acc<C, 5>(jacobian, points, terms, scalars, out_xy, out_inf, n) : wb == 8 ? mul_acc<C, 8>(jacobian, points, terms, scalars, out_xy, out_inf, n) : -1)
  return curve == 0 ? HT_MUL(CurveK256) : curve == 1 ? HT_MUL(CurveP256) : curve == 2 ? HT_MUL(CurveP384) : -1;
#undef HT_MUL
}
}
