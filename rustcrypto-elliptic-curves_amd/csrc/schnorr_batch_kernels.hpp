// BIP340 batch verification ("Batch Verification" of the BIP): u signatures hold together iff
//   sum_i a_i R_i + sum_i (a_i e_i) P_i - (sum_i a_i s_i) G = O
// for random coefficients a_i, R_i = lift_x(r_i), P_i = lift_x(pk_i).  This header turns a batch into the 2u + 1 terms of that sum in
// the layout CurveOps::msm reads (canonical big-endian scalars; affine x || y points); the sum itself is the library's MSM.
//   a_i = the first 16 bytes, big-endian, of SHA256(tag || tag || seed32 || be64(i)), tag = SHA256("ecgpu/BIP340/batch-coefficient"),
//         0 replaced by 1; i is the element's index in the CALLER's batch, so the coefficients do not depend on how a batch is cut.
//         The state after tag || tag is a constant: one compression per signature.
//   prep_kernel    one signature per lane: schnorr::decode and lift r (schnorr_kernels.hpp over affine_ops.hpp), write terms 2i = (a_i, R_i) and
//                  2i + 1 = (a_i e_i mod n, P_i), dec[i], and add t_i = a_i s_i mod n into the lane's wide accumulator.  An element
//                  that does not decode, or whose r is no x-coordinate, is invalid for the per-signature verifier as well (its R'
//                  is a curve point with x(R') = r): dec[i] = 0 and it is left out - scalars 0 on the point G, t_i = 0.
//                  The lanes' accumulators are added up deterministically: wave64 shuffles, LDS across the four waves, one partial
//                  per workgroup.  No atomics.
//   finish_kernel  one wave adds the partials, reduces (scops::reduce_wide) and writes term 2u = (n - sum mod n, G) and the number
//                  of elements with dec = 0.
// secp256k1 only.  The per-element functions are ECGPU_HD: tests/hosttwin/hosttwin_schnorr_batch.cpp compiles them for the host.
#pragma once
#include "h2c_hash.hpp"
#include "scalar_ops.hpp"
#include "schnorr_kernels.hpp"

namespace ecgpu {
namespace schnorr_batch {

// the state after the block tag || tag
static constexpr u32 COEFF_MID[8] = {0x99AB6236u, 0x9E518F4Bu, 0x7A1E7DEAu, 0x2994AA87u, 0x172826F1u, 0x0D70C2B1u, 0x5FCD1ECDu, 0x5D4C2192u};
// seed32 as the eight message words of the compression (big-endian words of the 32 bytes): a kernel argument
struct Seed {
  u32 w[8];
};
// a = the coefficient of element `index`, 8 little-endian limbs (the upper four are 0)
ECGPU_HD void coefficient(u32* a, const Seed& seed, u64 index) {
  using H = sha2::Sha256;
  u32 h[8], w[16];
#pragma unroll
  for (int i = 0; i < 8; i++) { h[i] = COEFF_MID[i]; w[i] = seed.w[i]; w[8 + i] = 0; }
  w[8] = (u32)(index >> 32);
  w[9] = (u32)index;
  w[10] = 0x80000000u;
  w[15] = (64 + 40) * 8;
  sha2::compress<H>(h, w);
  mp_zero<8>(a);
#pragma unroll
  for (int i = 0; i < 4; i++) a[i] = h[3 - i];
  if (mp_is_zero<8>(a)) a[0] = 1;
}

// Wide accumulators of the modular sum: SUMW words take 2^64 addends below 2^256 without a carry out.
constexpr int SUMW = 10;
// one partial of the sum as it lies in memory: the accumulator, then the number of left-out elements
constexpr int PARTIAL_WORDS = SUMW + 2;
// acc += t, t of TW words (8: a scalar, SUMW: another accumulator)
template <int TW>
ECGPU_HD void sum_add(u32* acc, const u32* t) {
  u32 c = 0;
#pragma unroll
  for (int i = 0; i < SUMW; i++) acc[i] = addc(acc[i], i < TW ? t[i] : 0u, c);
}
// k = n - (acc mod n), 0 where acc mod n = 0: the scalar of the generator term, limbs
ECGPU_HD void sum_finish(u32* k, const u32* acc) {
  using O = K256Order;
  u32 w[16], r[8];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = i < SUMW ? acc[i] : 0u;
  scops::reduce_wide<O>(r, w);
  smont::neg<O>(k, r);
}

// One signature.  px, sig, e: 8 / 16 / 8 words as they lie in memory.  Writes the two scalars (sc: 2 x 8 words) and the two points
// (pts: 2 x 16 words) of terms 2i and 2i + 1 in the MSM's wire layout and t = a s mod n (limbs; 0 for a left-out element).
// Returns dec: 1 where r in [1, p) is an x-coordinate, s in [1, n), the key x < p has a square root.
ECGPU_HD u32 prep_lane(u32* sc, u32* pts, u32* t, const u32* px, const u32* sig, const u32* e, const Seed& seed, u64 index) {
  using O = K256Order;
  u32 s[8], ee[8];
  FeK256 fr, yr, fx, yp;
  bool g = schnorr::decode(s, ee, fx, yp, px, sig, e);
  CurveK256::fe_load(fr, sig);
  g = schnorr::lift_even(yr, fr) && g;
  u32 a[8], ae[8];
  coefficient(a, seed, index);
  scops::mul_plain<O>(ae, a, ee);
  scops::mul_plain<O>(t, a, s);
  if (!g) {                                  // left out: 0 G + 0 G, t = 0
    PtK256 gen;
    k256::generator(gen);
    mp_zero<8>(a); mp_zero<8>(ae); mp_zero<8>(t);
    fr = gen.x; yr = gen.y; fx = gen.x; yp = gen.y;
  }
  words_store_be<8>(sc, a);
  words_store_be<8>(sc + 8, ae);
  CurveK256::fe_store(pts, fr);
  CurveK256::fe_store(pts + 8, yr);
  CurveK256::fe_store(pts + 16, fx);
  CurveK256::fe_store(pts + 24, yp);
  return g ? 1u : 0u;
}

// term 2u: (k, G) in the wire layout
ECGPU_HD void generator_term(u32* sc, u32* pts, const u32* k) {
  PtK256 gen;
  k256::generator(gen);
  words_store_be<8>(sc, k);
  CurveK256::fe_store(pts, gen.x);
  CurveK256::fe_store(pts + 8, gen.y);
}

}  // namespace schnorr_batch
}  // namespace ecgpu

#if defined(__HIPCC__)
#include "kernels.hpp"

namespace ecgpu {
namespace schnorr_batch {

// the accumulators of a wave added into its lane 0 (every lane of the wave calls this)
__device__ __forceinline__ void wave_sum(u32* acc, u32& bad) {
#pragma unroll 1
  for (int off = 32; off >= 1; off >>= 1) {
    u32 o[SUMW];
#pragma unroll
    for (int j = 0; j < SUMW; j++) o[j] = __shfl_down(acc[j], off);
    sum_add<SUMW>(acc, o);
    bad += __shfl_down(bad, off);
  }
}

// sc: (2n + 1) x 8 words, pts: (2n + 1) x 16 words (terms 0 .. 2n - 1 are written here), dec: n bytes,
// partial: gridDim.x x PARTIAL_WORDS words.  first_index: the caller's index of element 0.
template <int UNUSED>      // a template only so that the header can be included by every curve's translation unit
__global__ void __launch_bounds__(256) prep_kernel(const u32* px, const u32* sig, const u32* e, const Seed seed, u64 first_index, u32* sc, u32* pts,
                                                   uint8_t* dec, u32* partial, size_t n) {
  __shared__ u32 sh[4][PARTIAL_WORDS];
  u32 acc[SUMW], bad = 0;
#pragma unroll
  for (int j = 0; j < SUMW; j++) acc[j] = 0;
  ECGPU_GRID_STRIDE(i, n) {
    u32 s[16], p[32], t[8];
    const u32 g = prep_lane(s, p, t, px + i * 8, sig + i * 16, e + i * 8, seed, first_index + i);
    uint4* ds = (uint4*)(sc + i * 16);
    uint4* dp = (uint4*)(pts + i * 32);
#pragma unroll
    for (int q = 0; q < 4; q++) ds[q] = make_uint4(s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
#pragma unroll
    for (int q = 0; q < 8; q++) dp[q] = make_uint4(p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]);
    dec[i] = (uint8_t)g;
    bad += 1u - g;
    sum_add<8>(acc, t);
  }
  wave_sum(acc, bad);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < SUMW; j++) sh[wave][j] = acc[j];
    sh[wave][SUMW] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll 1
    for (int w = 1; w < 4; w++) { sum_add<SUMW>(acc, sh[w]); bad += sh[w][SUMW]; }
    u32* dst = partial + (size_t)blockIdx.x * PARTIAL_WORDS;
#pragma unroll
    for (int j = 0; j < SUMW; j++) dst[j] = acc[j];
    dst[SUMW] = bad;
    dst[SUMW + 1] = 0;
  }
}

// one wave: adds the `count` partials, writes term 2n (sc_last: 8 words, pts_last: 16 words) and the number of left-out elements
template <int UNUSED>
__global__ void __launch_bounds__(64) finish_kernel(const u32* partial, int count, u32* sc_last, u32* pts_last, u32* bad_out) {
  u32 acc[SUMW], bad = 0;
#pragma unroll
  for (int j = 0; j < SUMW; j++) acc[j] = 0;
#pragma unroll 1
  for (int b = threadIdx.x; b < count; b += 64) {
    const u32* src = partial + (size_t)b * PARTIAL_WORDS;
    sum_add<SUMW>(acc, src);
    bad += src[SUMW];
  }
  wave_sum(acc, bad);
  if (threadIdx.x == 0) {
    u32 k[8];
    sum_finish(k, acc);
    generator_term(sc_last, pts_last, k);
    *bad_out = bad;
  }
}

}  // namespace schnorr_batch
}  // namespace ecgpu
#endif
