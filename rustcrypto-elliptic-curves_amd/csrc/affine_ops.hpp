// Affine-point arithmetic shared by the kernels around the scalar multiplications (ECDSA verify and recover, BIP340 verify and
// batch verify, SEC1 decoding, decompression, point validation, the synthetic inputs): y from x, the curve check and the sum of
// two affine points with identity flags.  Written once over the curve traits; every function is ECGPU_HD, and
// tests/hosttwin/hosttwin_sigsum.cpp compiles them for the host, where the ECGPU_EXC_NOTE counters say which arm a pair entered.
#pragma once
#include "traits.hpp"

namespace ecgpu {
namespace aff {

// ---- y from x -------------------------------------------------------------------------------------------------------------------
// y, ny = the two square roots of x^3 + a x + b; returns whether they exist (the values mean nothing where they do not)
template <class C>
ECGPU_HD bool sqrt_rhs(typename C::Fe& y, typename C::Fe& ny, const typename C::Fe& x) {
  typename C::Fe rhs;
  C::curve_rhs(rhs, x);
  const bool has = C::fe_sqrt(y, rhs);
  ECGPU_EXC_NOTE("lift.no_root", !has);
  C::fe_neg(ny, y);
  return has;
}
// y = the root of the wanted parity
template <class C>
ECGPU_HD bool lift_x(typename C::Fe& y, const typename C::Fe& x, bool want_odd) {
  typename C::Fe ny;
  const bool has = sqrt_rhs<C>(y, ny, x);
  const bool odd = C::fe_is_odd(y);
  C::fe_select(y, odd == want_odd, y, ny);
  return has;
}

// ---- canonical and on the curve -------------------------------------------------------------------------------------------------
// every coordinate (NW big-endian words as they lie in memory) is below p: looks at the raw integers, before any domain conversion
template <class C>
ECGPU_HD bool coords_canonical(const u32* be) {
  u32 l[C::NW], p[C::NW];
  words_load_be<C::NW>(l, be);
  C::modulus(p);
  return !mp_geq<C::NW>(l, p);
}
template <class C, class... W>
ECGPU_HD bool coords_canonical(const u32* be, const W*... more) {
  return coords_canonical<C>(be) && coords_canonical<C>(more...);
}
// y^2 == x^3 + a x + b.  What the all-zero encoding means stays with the caller.
template <class C>
ECGPU_HD bool on_curve(const typename C::Fe& x, const typename C::Fe& y) {
  typename C::Fe l, r, d;
  C::fe_sqr(l, y);
  C::curve_rhs(r, x);
  C::fe_sub(d, l, r);
  return C::fe_is_zero(d);
}

// ---- A + B ------------------------------------------------------------------------------------------------------------------------
enum { SUM_NONE = 0, SUM_OPERAND = 1, SUM_CHORD = 2, SUM_TANGENT = 3 };      // two bits; kind & SUM_CHORD: a slope exists

template <class C>
ECGPU_HD bool same_coord(const u32* a, const u32* b) {
  bool same = true;
#pragma unroll
  for (int j = 0; j < C::NW; j++) same &= (a[j] == b[j]);
  return same;
}
// The kind of A + B for affine pa, pb (x || y as they lie in memory, canonical) and their identity flags:
//   SUM_NONE     the sum is the identity (both operands are, or A = -B)
//   SUM_OPERAND  one operand is the identity, the sum is the other
//   SUM_CHORD    different x
//   SUM_TANGENT  A = B (y != 0 on a curve of odd order)
template <class C>
ECGPU_HD u32 sum_kind(const u32* pa, bool a_inf, const u32* pb, bool b_inf) {
  if (a_inf && b_inf) { ECGPU_EXC_NOTE("affsum.both_inf", true); return SUM_NONE; }
  if (a_inf || b_inf) { ECGPU_EXC_NOTE("affsum.one_inf", true); return SUM_OPERAND; }
  const bool same_x = same_coord<C>(pa, pb), same_y = same_coord<C>(pa + C::NW, pb + C::NW);
  if (same_x && !same_y) { ECGPU_EXC_NOTE("affsum.opp", true); return SUM_NONE; }
  ECGPU_EXC_NOTE("affsum.same", same_x);
  ECGPU_EXC_NOTE("affsum.chord", !same_x);
  return same_x ? SUM_TANGENT : SUM_CHORD;
}
// The slope N / D of a SUM_CHORD or SUM_TANGENT (same_x) pair: tangent 3 x^2 + a over 2 y, chord yB - yA over xB - xA
template <class C>
ECGPU_HD void slope_terms(typename C::Fe& N, typename C::Fe& D, const typename C::Fe& xa, const typename C::Fe& ya, const typename C::Fe& xb,
                          const typename C::Fe& yb, bool same_x) {
  if (same_x) {
    typename C::Fe t;
    C::fe_sqr(t, xa);
    if (!C::A_IS_ZERO) { typename C::Fe one; C::fe_one(one); C::fe_sub(t, t, one); }      // a = -3: 3 (x^2 - 1)
    C::fe_add(N, t, t); C::fe_add(N, N, t);
    C::fe_add(D, ya, ya);
  } else {
    C::fe_sub(N, yb, ya);
    C::fe_sub(D, xb, xa);
  }
}
// D of slope_terms alone, loading only the coordinates it needs: all that the forward pass of sum_batch wants of a pair (with
// slope_terms there, P-256's recover_finish_kernel took 8 more VGPRs than with its own copy of these two lines)
template <class C>
ECGPU_HD void slope_den(typename C::Fe& D, const u32* pa, const u32* pb, bool same_x) {
  typename C::Fe u, v;
  if (same_x) { C::fe_load(u, pa + C::NW); C::fe_add(D, u, u); }
  else { C::fe_load(u, pa); C::fe_load(v, pb); C::fe_sub(D, v, u); }
}

// A + B for the up to BATCH elements base, base + T, base + 2 T, .. below n - one lane's share of a grid-stride walk - with one field
// inversion (Montgomery's trick): the forward pass multiplies the denominators of the chords and tangents together, the backward pass
// unwinds.  An element with ok[i] = 0 counts as SUM_NONE; only chords and tangents enter the product.  emit(i, kind, x3, y3) gets
// every element once, last first, x3 = y3 = 0 for SUM_NONE, and may write ok[i].
template <class C, int BATCH, class Emit>
ECGPU_HD void sum_batch(const u32* a_xy, const uint8_t* a_inf, const u32* b_xy, const uint8_t* b_inf, const uint8_t* ok, size_t base, size_t T, size_t n,
                        Emit emit) {
  using Fe = typename C::Fe;
  constexpr int L = C::NW;
  Fe pre[BATCH];
  u32 kinds = 0;          // two bits per element
  int cnt = 0;
  Fe acc; C::fe_one(acc);
#pragma unroll 1
  for (int b = 0; b < BATCH; b++) {
    const size_t i = base + (size_t)b * T;
    if (i >= n) break;
    cnt = b + 1;
    pre[b] = acc;
    if (!ok[i]) continue;
    const u32* pa = a_xy + i * 2 * L;
    const u32* pb = b_xy + i * 2 * L;
    const u32 kind = sum_kind<C>(pa, a_inf[i] != 0, pb, b_inf[i] != 0);
    kinds |= kind << (2 * b);
    if (!(kind & SUM_CHORD)) continue;
    Fe D;
    slope_den<C>(D, pa, pb, kind == SUM_TANGENT);
    C::fe_mul(acc, acc, D);
  }
  Fe inv_all;
  C::fe_inv(inv_all, acc);
#pragma unroll 1
  for (int b = cnt - 1; b >= 0; b--) {
    const size_t i = base + (size_t)b * T;
    const u32 kind = (kinds >> (2 * b)) & 3u;
    const u32* pa = a_xy + i * 2 * L;
    const u32* pb = b_xy + i * 2 * L;
    Fe x3, y3;
    C::fe_zero(x3); C::fe_zero(y3);
    if (kind == SUM_OPERAND) {
      const u32* src = a_inf[i] ? pb : pa;
      C::fe_load(x3, src);
      C::fe_load(y3, src + L);
    } else if (kind & SUM_CHORD) {
      Fe xa, ya, xb, yb, N, D, di, lam, t;
      C::fe_load(xa, pa); C::fe_load(ya, pa + L);
      C::fe_load(xb, pb); C::fe_load(yb, pb + L);
      slope_terms<C>(N, D, xa, ya, xb, yb, kind == SUM_TANGENT);
      C::fe_mul(di, inv_all, pre[b]);                   // 1 / D
      C::fe_mul(inv_all, inv_all, D);
      C::fe_mul(lam, N, di);
      C::fe_sqr(x3, lam);
      C::fe_sub(x3, x3, xa); C::fe_sub(x3, x3, xb);
      C::fe_sub(t, xa, x3);
      C::fe_mul(y3, lam, t);
      C::fe_sub(y3, y3, ya);
    }
    emit(i, kind, x3, y3);
  }
}

}  // namespace aff
}  // namespace ecgpu
