// BIP340 Schnorr verification for batches: the elliptic-curve part of
// `VerifyingKey::verify_prehash` (k256/src/schnorr/verifying.rs:62-93).
//   e = tagged_hash("BIP0340/challenge", r || P.x || m) mod n comes from the caller (ecgpu_schnorr_verify_batch) or from the
//   challenge kernel of h2c_hash.hpp (ecgpu_schnorr_verify_prehash_batch);
//   R = s G + (-e) P must be finite, have even y and x(R) = r.
// Pipeline: verify_prep (decode r, s, lift_x of the key, -e) -> fixed-base kernel (s G) -> variable-base kernel
// ((-e) P) -> verify_check (affine sum with one inversion per BATCH signatures, parity and x tests).
// secp256k1 only.  decode is ECGPU_HD (schnorr_batch_kernels.hpp, which builds for the host, shares it); the kernels are device code.
#pragma once
#include "affine_ops.hpp"

namespace ecgpu {
namespace schnorr {

// BIP340's lift_x: y = the even root of x^3 + 7; returns whether there is one.  (A conditional copy, not aff::lift_x's select with a
// constant parity: with the select schnorr_batch::prep_kernel takes 180 VGPRs in place of 172.)
ECGPU_HD bool lift_even(FeK256& y, const FeK256& x) {
  FeK256 ny;
  const bool has = aff::sqrt_rhs<CurveK256>(y, ny, x);
  if (k256::is_odd(y)) y = ny;
  return has;
}

// decode: r in [1, p) (Signature::try_from, k256/src/schnorr.rs:142-160), s in [1, n), key x < p with a square root
// (VerifyingKey::from_bytes -> decompact, verifying.rs:39-45).  px, sig, e: 8 / 16 / 8 words as they lie in memory.  Gives s and
// e mod n (limbs; Reduce::reduce_bytes of the challenge hash) and P = (fx, even y); returns whether the element decodes.
ECGPU_HD bool decode(u32* s, u32* ee, FeK256& fx, FeK256& y, const u32* px, const u32* sig, const u32* e) {
  u32 r[8], ord[8];
  words_load_be<8>(r, sig);
  words_load_be<8>(s, sig + 8);
  words_load_be<8>(ee, e);
  k256::order(ord);
  bool g = !mp_is_zero<8>(r) && !mp_is_zero<8>(s) && !mp_geq<8>(s, ord) && aff::coords_canonical<CurveK256>(sig, px);
  CurveK256::fe_load(fx, px);
  g = lift_even(y, fx) && g;
  k256::scalar_reduce_once(ee);
  return g;
}

}  // namespace schnorr
}  // namespace ecgpu

#if defined(__HIPCC__)
#include "kernels.hpp"

namespace ecgpu {
namespace schnorr {

// Writes P = (x, even y), u1 = s, u2 = -e mod n.
template <int UNUSED>      // a template only so that the header can be included by every curve's translation unit
__global__ void __launch_bounds__(256) verify_prep_kernel(const u32* px, const u32* sig, const u32* e, u32* p_xy, u32* u1, u32* u2, uint8_t* ok,
                                                          size_t n) {
  ECGPU_GRID_STRIDE(i, n) {
    u32 s[8], ee[8], ord[8], me[8];
    FeK256 fx, y;
    const bool g = decode(s, ee, fx, y, px + i * 8, sig + i * 16, e + i * 8);
    k256::order(ord);
    mp_sub<8>(me, ord, ee);                  // -e  (0 stays 0)
    if (mp_is_zero<8>(ee)) mp_zero<8>(me);
    if (!g) { mp_zero<8>(s); mp_zero<8>(me); k256::set_zero(fx); k256::set_zero(y); }
    CurveK256::fe_store(p_xy + i * 16, fx);
    CurveK256::fe_store(p_xy + i * 16 + 8, y);
    words_store_be<8>(u1 + i * 8, s);
    words_store_be<8>(u2 + i * 8, me);
    ok[i] = g ? 1 : 0;
  }
}

// R = A + B in affine coordinates (one inversion per BATCH signatures); valid iff R is finite, y(R) is even and x(R) = r.
template <int BATCH>
__global__ void __launch_bounds__(256) verify_check_kernel(const u32* a_xy, const uint8_t* a_inf, const u32* b_xy, const uint8_t* b_inf,
                                                           const u32* sig, uint8_t* ok, size_t n) {
  using C = CurveK256;
  const size_t T = (size_t)gridDim.x * blockDim.x;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t base = tid; base < n; base += T * BATCH) {
    aff::sum_batch<C, BATCH>(a_xy, a_inf, b_xy, b_inf, ok, base, T, n, [&](size_t i, u32 kind, const FeK256& x3, const FeK256& y3) {
      bool valid = kind != aff::SUM_NONE;
      if (valid) {
        FeK256 r, d;
        C::fe_load(r, sig + i * 16);
        C::fe_sub(d, x3, r);
        valid = C::fe_is_zero(d) && !C::fe_is_odd(y3);
      }
      ok[i] = valid ? 1 : 0;
    });
  }
}

}  // namespace schnorr
}  // namespace ecgpu
#endif
