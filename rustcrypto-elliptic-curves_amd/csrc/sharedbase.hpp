// Shared points (ECGPU_SHARED_POINTS): one point H per batch, multiplied from a cached digit-indexed table like the generator.
//
// The table has the generator tables' layout, so the fixed-base kernels read it as they read theirs (fixedbase.hpp,
// fixedbase_ct.hpp): T[j][d-1] = d 2^(WB j) H as AffEntry<C> in the internal field form, nwin_wide<C, WB>() windows of
// wide_entries<WB>() entries, WB = 5 (the constant-time kernel's), 8, 16 or 20.  The generator tables are built by multiplying G
// with the scalars d 2^(WB j) on the 8-bit generator kernel, which no other base can use; these are built from H itself:
//   stage A  lane j: B_j = 2^(WB j) H by doublings, normalised (shared_window_base);
//   stage B  one lane per run of SHARED_RUN consecutive multiples of one window (shared_run): the first multiple by
//            double-and-add on the small integer, fifteen mixed additions of the affine B_j, one shared inversion.
// Both bodies, and the per-result body of the multi-table kernel (mul_shared_one), are host + device: the host twin walks them.
#pragma once
#include "jacobian.hpp"
#include "fixedbase_ct.hpp"      // the tables' geometry

namespace ecgpu {
namespace fb {

constexpr int SHARED_MAX_TERMS = 8;        // tables one launch of the multi-table kernel reads (its argument block holds the pointers)
constexpr int SHARED_RUN = 16;             // consecutive multiples per lane of stage B: divides wide_entries<WB>() for every WB >= 5

// the tables of one call; a null pointer is a term whose point is the identity: it contributes nothing
template <class C>
struct SharedTabs {
  const AffEntry<C>* t[SHARED_MAX_TERMS];
  int terms;
};

// stage A: b = 2^doublings h, affine.  h is a point of the curve and not the identity, so neither is any 2^i h (odd prime order).
template <class C>
ECGPU_HD void shared_window_base(AffEntry<C>& b, const AffEntry<C>& h, int doublings) {
  using Fe = typename C::Fe;
  Jac<C> p;
  p.x = h.x; p.y = h.y; C::fe_one(p.z);
#pragma unroll 1
  for (int i = 0; i < doublings; i++) jac::dbl<C>(p);
  Fe zi, t;
  C::fe_inv(zi, p.z);
  C::fe_sqr(t, zi);
  C::fe_mul(b.x, p.x, t);
  C::fe_mul(t, t, zi);
  C::fe_mul(b.y, p.y, t);
}

// stage B: out[i] = (first + i) b, i < SHARED_RUN, affine.  The step 1 b + b (first = 1) takes jac::add_mixed's doubling branch; for a
// base of order n no other step of the chain is exceptional (m b = +-b needs n | m -+ 1, and m < 2^20), but nothing here relies on
// that: every addition resolves its special operands by control flow, and a multiple that came out as the identity is written as zeros
// and kept out of the shared inversion.
template <class C>
ECGPU_HD void shared_run(AffEntry<C>* out, const AffEntry<C>& b, u32 first) {
  using Fe = typename C::Fe;
  Jac<C> run[SHARED_RUN];
  Fe pre[SHARED_RUN];
  Jac<C> acc;
  acc.x = b.x; acc.y = b.y; C::fe_one(acc.z);
  int top = 0;
  while ((first >> (top + 1)) != 0) top++;
#pragma unroll 1
  for (int bit = top - 1; bit >= 0; bit--) {
    jac::dbl<C>(acc);
    if ((first >> bit) & 1u) jac::add_mixed<C>(acc, b.x, b.y);
  }
  run[0] = acc;
#pragma unroll 1
  for (int i = 1; i < SHARED_RUN; i++) {
    jac::add_mixed<C>(acc, b.x, b.y);
    run[i] = acc;
  }
  Fe prod, one;
  C::fe_one(prod); C::fe_one(one);
#pragma unroll 1
  for (int i = 0; i < SHARED_RUN; i++) {
    pre[i] = prod;
    if (C::fe_is_zero(run[i].z)) continue;
    C::fe_mul(prod, prod, run[i].z);
  }
  Fe inv;
  C::fe_inv(inv, prod);
#pragma unroll 1
  for (int i = SHARED_RUN - 1; i >= 0; i--) {
    if (C::fe_is_zero(run[i].z)) { C::fe_zero(out[i].x); C::fe_zero(out[i].y); continue; }
    Fe zi, t;
    C::fe_mul(zi, inv, pre[i]);
    C::fe_mul(inv, inv, run[i].z);
    C::fe_sqr(t, zi);
    C::fe_mul(out[i].x, run[i].x, t);
    C::fe_mul(t, t, zi);
    C::fe_mul(out[i].y, run[i].y, t);
  }
}

// acc = sum_t k_t H_t over the tables of `tabs`: the window loop of fb::mul_wide_kernel once per term, all terms into ONE accumulator
// (Acc is fixedbase.hpp's FbAcc<C>: XYZZ on the 256-bit curves, Jacobian on P-384).  sc: the element's terms scalars, canonical
// big-endian words.  Every term folds its scalar to min(k, n - k) (the entries' sign absorbs the flip) and has its own recoding carry.
// Unlike the single-base loop this one DOES meet the additions' exceptional operands - H_2 = +-H_1, H_2 = 2 H_1, partial sums that are
// the identity - and leaves them to the control flow of Acc::add_mixed / Acc::add_affine.  `filled` = 1 marks an accumulator that is
// one affine entry (Z = 1: the cheaper add_affine applies); it is set only by the addition into the EMPTY accumulator and cleared by the
// next one, whatever that one's outcome (an accumulator that returns to the identity later is add_mixed's own special case).
template <class C, int WB, class Acc>
ECGPU_HD void mul_shared_one(typename Acc::Pt& acc, const u32* sc, const SharedTabs<C>& tabs) {
  constexpr int NW = C::NW, NWIN = nwin_wide<C, WB>();
  Acc::set_infinity(acc);
  int filled = 0;
#pragma unroll 1
  for (int t = 0; t < tabs.terms; t++) {
    const AffEntry<C>* table = tabs.t[t];
    if (!table) continue;
    u32 k[NW], ord[NW], f[NW];
    C::scalar_load(k, sc + t * NW);
    C::order(ord);
    reduce_once<NW>(k, ord);
    mp_sub<NW>(f, ord, k);
    const bool flip = !mp_geq<NW>(f, k);              // n - k < k
#pragma unroll
    for (int w = 0; w < NW; w++) k[w] = flip ? f[w] : k[w];
    u32 carry = 0;
#pragma unroll 1
    for (int j = 0; j < NWIN; j++) {
      const int wi = (WB * j) >> 5, sh = (WB * j) & 31;
      u32 w0 = 0, w1 = 0;
#pragma unroll
      for (int q = 0; q < NW; q++) { w0 = (wi == q) ? k[q] : w0; w1 = (wi + 1 == q) ? k[q] : w1; }
      const u64 pair = ((u64)w1 << 32) | w0;
      const u32 d = ((u32)(pair >> sh) & ((1u << WB) - 1u)) + carry;
      carry = (d >= (1u << (WB - 1))) ? 1u : 0u;       // d in [2^(WB-1), 2^WB] becomes d - 2^WB with a carry
      const int sd = (int)d - (int)(carry << WB);
      if (sd == 0) continue;
      const int e_idx = j * wide_entries<WB>() + ((sd < 0 ? -sd : sd) - 1);
      ECGPU_TABLE_TOUCH(t * NWIN * wide_entries<WB>() + e_idx);
      const AffEntry<C>* e = table + e_idx;
      typename C::Fe x = e->x, y = e->y;
      if ((sd < 0) != flip) C::fe_neg(y, y);
      if (filled == 1) { Acc::add_affine(acc, x, y); filled = 2; }
      else { Acc::add_mixed(acc, x, y); filled = filled ? 2 : 1; }
    }
  }
}

}  // namespace fb
}  // namespace ecgpu
