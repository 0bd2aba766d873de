// TEST-ONLY op table over the point formulas (csrc/jacobian.hpp, msm.hpp, mulfast_k256.hpp) and the masked additions of the
// constant-time kernels (varbase_ct_k256.hpp, varbase_ct.hpp, fixedbase_ct.hpp: the very functions their window loops call), one
// pair of operands per call.  The same
// functions are compiled for gfx950 into tests/devtwin (devtwin_group.hip: one pair per lane, so a wave's lanes can disagree
// about the branch they take) and for the host into tests/hosttwin (hosttwin_group.cpp: the ECGPU_EXC_NOTE counters say which
// branch a vector reached).  Operands and results are the field's internal words, raw and little-endian, with no conversion
// on entry or exit: raw (possibly >= p) values for secp256k1, Montgomery form for P-256 / P-384.  Never linked into libecgpu.so.
#pragma once
#include "traits.hpp"
#include "jacobian.hpp"
#include "msm.hpp"
#include "mulfast_k256.hpp"
#include "varbase_ct.hpp"
#include "varbase_ct_k256.hpp"
#include "fixedbase_ct.hpp"

namespace ecgpu {
namespace twin {

// per pair: p and q are PT_IN_FE field elements each, aux PT_AUX words, out PT_OUT_FE field elements and a flag word.
//   Jacobian operand: X, Y, Z;  XYZZ operand: X, Y, ZZ, ZZZ;  affine operand: x, y.  Unused elements are ignored / written as zero.
//   aux[0]: the `empty` mask, aux[1]: the zero-digit mask of the masked forms (all ones or zero).
constexpr int PT_IN_FE = 4, PT_OUT_FE = 5, PT_AUX = 2;
template <class C> constexpr int pt_out_words() { return PT_OUT_FE * C::NW + 1; }

enum PtOp {
  // every curve.  out: the Jacobian triple in elements 0..2, or the XYZZ quadruple in 0..3
  G_DBL,                 // jac::dbl(p)
  G_ADD_MIXED,           // jac::add_mixed(p, q affine)
  G_ADD_AFFINE,          // jac::add_affine((p.X, p.Y, 1), q affine)
  G_ADD,                 // jac::add(p, q)
  G_XYZZ_ADD_MIXED,      // msm::xyzz_add_mixed(p, q affine)
  G_XYZZ_ADD_AFFINE,     // msm::xyzz_add_affine((p.X, p.Y, 1, 1), q affine)
  G_XYZZ_ADD,            // msm::xyzz_add(p, q)
  G_XYZZ_ROUNDTRIP,      // jacobian_to_xyzz(p) then xyzz_to_jacobian: the triple in 0..2, the ZZZ in between in 3
  // the masked addition that fb::mul_ct_one calls for every digit: fb::xyzz_ct_accumulate(p, empty, q affine, |digit|, one).
  // flag: `empty` afterwards
  M_FB_ACCUMULATE,
  // the masked addition that vbct::lane_pass calls for every digit (P-256 / P-384: fully reduced fields):
  // vbct::ct_accumulate(p, empty, q affine, zd, one).  flag bit 0: `empty` afterwards, bit 1: fe_zero_mask of the resulting Z
  M_VBCT_ACCUMULATE,
  // secp256k1 only
  K_JAC_ADD_MIXED,       // k256::jac_add_mixed(p, q affine, &zr): zr in element 4
  K_JAC_ADD_MIXED_NEG,   // k256::jac_add_mixed_neg(p, q affine)
  K_JAC_DOUBLE,          // k256::jac_double(p)
  K_JAC_DOUBLE_NEG,      // k256::jac_double_neg(p)
  K_JAC_DOUBLE_AFFINE,   // k256::jac_double_affine(p.X, p.Y)
  K_COZ_DOUBLE_AFFINE,   // k256::coz_double_affine(p.X, p.Y): d in 0..2, (qx, qy) in 3, 4
  K_COZ_ADD_UPDATE,      // k256::coz_add_update(r = (p.X, p.Y), q = (q.X, q.Y)): r in 0, 1, h in 2, q in 3, 4
  K_ADD_MIXED_RAW,       // vbct::k256_add_mixed_raw(p, q affine, &zr): zr in element 4
  K_CT_ACCUMULATE,       // vbct::k256_ct_accumulate(p, empty, q affine, zd, one).  flag: `empty` afterwards
  K_JAC_ADD_MIXED_NOZR,  // k256::jac_add_mixed(p, q affine, nullptr): the form every kernel calls; element 4 stays zero
  PT_NOPS
};

template <class Fe, int NW>
ECGPU_HD void pt_load(Fe& r, const u32* w) {
#pragma unroll
  for (int i = 0; i < NW; i++) r.v[i] = w[i];
}

// the secp256k1 forms of mulfast_k256.hpp and varbase_ct_k256.hpp
ECGPU_HD bool k256_pt_op(int op, const FeK256* p, const FeK256* q, const u32* aux, FeK256* o, u32& flag) {
  JacK256 a;
  a.x = p[0]; a.y = p[1]; a.z = p[2];
  switch (op) {
    case K_JAC_ADD_MIXED: k256::jac_add_mixed(a, q[0], q[1], &o[4]); break;
    case K_JAC_ADD_MIXED_NOZR: k256::jac_add_mixed(a, q[0], q[1], nullptr); break;
    case K_JAC_ADD_MIXED_NEG: k256::jac_add_mixed_neg(a, q[0], q[1]); break;
    case K_JAC_DOUBLE: k256::jac_double(a); break;
    case K_JAC_DOUBLE_NEG: k256::jac_double_neg(a); break;
    case K_JAC_DOUBLE_AFFINE: k256::jac_double_affine(a, p[0], p[1]); break;
    case K_COZ_DOUBLE_AFFINE: k256::coz_double_affine(a, o[3], o[4], p[0], p[1]); break;
    case K_COZ_ADD_UPDATE:
      o[3] = q[0]; o[4] = q[1];
      k256::coz_add_update(a.x, a.y, o[3], o[4], a.z);
      break;
    case K_ADD_MIXED_RAW: vbct::k256_add_mixed_raw(a, q[0], q[1], &o[4]); break;
    case K_CT_ACCUMULATE: {
      FeK256 one;
      k256::set_one(one);
      u32 empty = aux[0];
      vbct::k256_ct_accumulate(a, empty, q[0], q[1], aux[1], one);
      flag = empty;
      break;
    }
    default: return false;
  }
  o[0] = a.x; o[1] = a.y; o[2] = a.z;
  return true;
}

template <class C>
ECGPU_HD bool pt_op(int op, const u32* p, const u32* q, const u32* aux, u32* out) {
  using Fe = typename C::Fe;
  constexpr int NW = C::NW;
  Fe pi[PT_IN_FE], qi[PT_IN_FE], o[PT_OUT_FE];
#pragma unroll
  for (int e = 0; e < PT_IN_FE; e++) { pt_load<Fe, NW>(pi[e], p + e * NW); pt_load<Fe, NW>(qi[e], q + e * NW); }
#pragma unroll
  for (int e = 0; e < PT_OUT_FE; e++) C::fe_zero(o[e]);
  u32 flag = 0;
  bool ok = true;
  if (op >= K_JAC_ADD_MIXED) {
    if constexpr (C::A_IS_ZERO) ok = k256_pt_op(op, pi, qi, aux, o, flag);
    else ok = false;
  } else if (op <= G_ADD || op == G_XYZZ_ROUNDTRIP || op == M_VBCT_ACCUMULATE) {
    Jac<C> a, b;
    a.x = pi[0]; a.y = pi[1]; a.z = pi[2];
    b.x = qi[0]; b.y = qi[1]; b.z = qi[2];
    switch (op) {
      case G_DBL: jac::dbl<C>(a); break;
      case G_ADD_MIXED: jac::add_mixed<C>(a, qi[0], qi[1]); break;
      case G_ADD_AFFINE: C::fe_one(a.z); jac::add_affine<C>(a, qi[0], qi[1]); break;
      case G_ADD: { Jac<C> r; jac::add<C>(r, a, b); a = r; break; }
      case G_XYZZ_ROUNDTRIP: {
        msm::Xyzz<C> t;
        msm::jacobian_to_xyzz<C>(t, a);
        o[3] = t.zzz;
        msm::xyzz_to_jacobian<C>(a, t);
        break;
      }
      default:                                   // M_VBCT_ACCUMULATE
        if constexpr (!C::A_IS_ZERO) {
          Fe one;
          C::fe_one(one);
          u32 empty = aux[0];
          vbct::ct_accumulate<C>(a, empty, qi[0], qi[1], aux[1], one);
          flag = (empty & 1u) | (vbct::fe_zero_mask<C>(a.z) & 2u);
        } else {
          ok = false;
        }
    }
    o[0] = a.x; o[1] = a.y; o[2] = a.z;
  } else {
    msm::Xyzz<C> a, b;
    a.x = pi[0]; a.y = pi[1]; a.zz = pi[2]; a.zzz = pi[3];
    b.x = qi[0]; b.y = qi[1]; b.zz = qi[2]; b.zzz = qi[3];
    switch (op) {
      case G_XYZZ_ADD_MIXED: msm::xyzz_add_mixed<C>(a, qi[0], qi[1]); break;
      case G_XYZZ_ADD_AFFINE: C::fe_one(a.zz); C::fe_one(a.zzz); msm::xyzz_add_affine<C>(a, qi[0], qi[1]); break;
      case G_XYZZ_ADD: msm::xyzz_add<C>(a, b); break;
      case M_FB_ACCUMULATE: {                    // aux[1] is the zero-digit mask: magnitude 0 for a zero digit, 1 for any other
        Fe one;
        C::fe_one(one);
        u32 empty = aux[0];
        fb::xyzz_ct_accumulate<C>(a, empty, qi[0], qi[1], ~aux[1] & 1u, one);
        flag = empty;
        break;
      }
      default: ok = false;
    }
    o[0] = a.x; o[1] = a.y; o[2] = a.zz; o[3] = a.zzz;
  }
#pragma unroll
  for (int e = 0; e < PT_OUT_FE; e++)
#pragma unroll
    for (int w = 0; w < NW; w++) out[e * NW + w] = o[e].v[w];
  out[PT_OUT_FE * NW] = flag;
  return ok;
}

}  // namespace twin
}  // namespace ecgpu
