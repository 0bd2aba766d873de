// TEST-ONLY element-wise op tables over the field and scalar primitives (csrc/fe_k256.hpp, fe_mont.hpp, scalar_mont.hpp,
// mp32.hpp: mac_cols).  The same functions are compiled for gfx950 into tests/devtwin (the inline-asm column forms of
// mp32_cols.inc) and for the host into tests/hosttwin (the portable fallback), so one op table runs on both sides.
// Operands and results are raw little-endian 32-bit words, with no conversion on entry or exit.  Never linked into libecgpu.so.
#pragma once
#include "fe_k256.hpp"
#include "fe_mont.hpp"
#include "scalar_mont.hpp"

namespace ecgpu {
namespace twin {

// k256 ops on raw 256-bit operands (possibly >= p); the result is the raw, weakly reduced value (not normalised).
// out: 8 result words and a flag word (sqrt: is a root; is_zero_fast: the answer; 0 otherwise).
enum K256Op {
  K_MUL, K_SQR, K_ADD, K_SUB, K_NEG, K_INV, K_SQRT, K_MUL_SMALL,   // mul_small(a, b[0])
  K_SHL1, K_SHL2, K_SHL3,                                          // shl<3> runs aliased (r == a)
  K_MUL_ADD2,                                                      // a b + e f
  K_MUL_ADD_SQR,                                                   // a b + e^2
  K_HALF, K_SUB2,                                                  // sub2: a - b - e
  K_NORMALIZE,
  K_FOLD_TOP_FAST,                                                 // a + T C, T = b[0] + 2^32 (b[1] & 0xFF) < 2^40
  K_IS_ZERO_FAST,
  K_NOPS
};
ECGPU_HD bool k256_op(int op, const u32* a, const u32* b, const u32* e, const u32* f, u32* out) {
  FeK256 x, y, u, v, r;
  for (int i = 0; i < 8; i++) { x.v[i] = a[i]; y.v[i] = b[i]; u.v[i] = e[i]; v.v[i] = f[i]; }
  u32 flag = 0;
  switch (op) {
    case K_MUL: k256::mul(r, x, y); break;
    case K_SQR: k256::sqr(r, x); break;
    case K_ADD: k256::add(r, x, y); break;
    case K_SUB: k256::sub(r, x, y); break;
    case K_NEG: k256::neg(r, x); break;
    case K_INV: k256::inv(r, x); break;
    case K_SQRT: flag = k256::sqrt(r, x) ? 1u : 0u; break;
    case K_MUL_SMALL: k256::mul_small(r, x, y.v[0]); break;
    case K_SHL1: k256::shl<1>(r, x); break;
    case K_SHL2: k256::shl<2>(r, x); break;
    case K_SHL3: r = x; k256::shl<3>(r, r); break;
    case K_MUL_ADD2: k256::mul_add2(r, x, y, u, v); break;
    case K_MUL_ADD_SQR: k256::mul_add_sqr(r, x, y, u); break;
    case K_HALF: k256::half(r, x); break;
    case K_SUB2: k256::sub2(r, x, y, u); break;
    case K_NORMALIZE: k256::normalize(r, x); break;
    case K_FOLD_TOP_FAST: r = x; k256::fold_top_fast(r.v, (u64)y.v[0] | ((u64)(y.v[1] & 0xFFu) << 32)); break;
    case K_IS_ZERO_FAST: r = x; flag = k256::is_zero_fast(x) ? 1u : 0u; break;
    default: return false;
  }
  for (int i = 0; i < 8; i++) out[i] = r.v[i];
  out[8] = flag;
  return true;
}

// FeMont<P256Mod | P384Mod> ops on the internal (Montgomery-form) words as given; to_mont takes a canonical integer and
// from_mont returns one.  out: N result words and a flag word (sqrt: is a root; 0 otherwise).
enum MontOp { M_MUL, M_SQR, M_ADD, M_SUB, M_NEG, M_DBL, M_HALF, M_TO_MONT, M_FROM_MONT, M_INV, M_SQRT, M_NOPS };
template <class M>
ECGPU_HD bool mont_op(int op, const u32* a, const u32* b, u32* out) {
  constexpr int N = M::N;
  FeMont<M> x, y, r;
  for (int i = 0; i < N; i++) { x.v[i] = a[i]; y.v[i] = b[i]; }
  u32 flag = 0;
  switch (op) {
    case M_MUL: mont::mul(r, x, y); break;
    case M_SQR: mont::sqr(r, x); break;
    case M_ADD: mont::add(r, x, y); break;
    case M_SUB: mont::sub(r, x, y); break;
    case M_NEG: mont::neg(r, x); break;
    case M_DBL: mont::dbl(r, x); break;
    case M_HALF: mont::half(r, x); break;
    case M_TO_MONT: mont::to_mont(r, x.v); break;
    case M_FROM_MONT: mont::from_mont(r.v, x); break;
    case M_INV: mont::inv(r, x); break;
    case M_SQRT: flag = mont::sqrt(r, x) ? 1u : 0u; break;
    default: return false;
  }
  for (int i = 0; i < N; i++) out[i] = r.v[i];
  out[N] = flag;
  return true;
}

// smont ops for the group orders; reduce_once(a) works on a copy.  out: L result words.
enum ScalarOp { S_MUL, S_ADD, S_REDUCE_ONCE, S_TO_MONT, S_FROM_MONT, S_INV, S_NOPS };
template <class O>
ECGPU_HD bool scalar_op(int op, const u32* a, const u32* b, u32* out) {
  constexpr int L = O::L;
  u32 x[L], y[L], r[L];
  for (int i = 0; i < L; i++) { x[i] = a[i]; y[i] = b[i]; }
  switch (op) {
    case S_MUL: smont::mul<O>(r, x, y); break;
    case S_ADD: smont::add<O>(r, x, y); break;
    case S_REDUCE_ONCE: mp_copy<L>(r, x); smont::reduce_once<O>(r); break;
    case S_TO_MONT: smont::to_mont<O>(r, x); break;
    case S_FROM_MONT: smont::from_mont<O>(r, x); break;
    case S_INV: smont::inv<O>(r, x); break;
    default: return false;
  }
  for (int i = 0; i < L; i++) out[i] = r[i];
  return true;
}

// mac_cols<M, FRESH, NC>(c, pa, pb) for M = 1..13 (13: the split at 12), FRESH in {0, 1}, NC in {0, 1, 2} with NC <= M.
// c: 3 words (c.lo low, c.lo high, c.hi) in and out; pa, pb: MAC_MAX_M words each.  FRESH needs c.hi == 0 on entry, and the
// first NC products must not carry out of c.lo: the caller's inputs state both, as at the call sites.
constexpr int MAC_MAX_M = 13;
template <int M, bool FRESH>
ECGPU_HD bool mac_cols_nc_dispatch(int nc, Acc96& c, const u32* pa, const u32* pb) {
  if (nc == 0) { mac_cols<M, FRESH, 0>(c, pa, pb); return true; }
  if (nc == 1) { mac_cols<M, FRESH, 1>(c, pa, pb); return true; }
  if constexpr (M >= 2) {
    if (nc == 2) { mac_cols<M, FRESH, 2>(c, pa, pb); return true; }
  }
  return false;
}
template <int M>
ECGPU_HD bool mac_cols_dispatch(int m, int fresh, int nc, Acc96& c, const u32* pa, const u32* pb) {
  if (m == M) return fresh ? mac_cols_nc_dispatch<M, true>(nc, c, pa, pb) : mac_cols_nc_dispatch<M, false>(nc, c, pa, pb);
  if constexpr (M < MAC_MAX_M) return mac_cols_dispatch<M + 1>(m, fresh, nc, c, pa, pb);
  return false;
}
ECGPU_HD bool mac_cols_op(int m, int fresh, int nc, const u32* c_in, const u32* pa, const u32* pb, u32* out) {
  Acc96 c;
  c.lo = (u64)c_in[0] | ((u64)c_in[1] << 32);
  c.hi = c_in[2];
  if (!mac_cols_dispatch<1>(m, fresh, nc, c, pa, pb)) return false;
  out[0] = (u32)c.lo;
  out[1] = (u32)(c.lo >> 32);
  out[2] = c.hi;
  return true;
}
ECGPU_HD bool mac_cols_valid(int m, int fresh, int nc) {
  return m >= 1 && m <= MAC_MAX_M && (fresh == 0 || fresh == 1) && nc >= 0 && nc <= 2 && nc <= m;
}

}  // namespace twin
}  // namespace ecgpu
