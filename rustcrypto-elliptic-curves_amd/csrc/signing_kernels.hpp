// Deterministic signing on the device: the secret nonce comes from the key and the digest alone.
//   ECDSA  - SigningKey::sign_prehash / RandomizedPrehashSigner of the external ecdsa crate (k256 | p256 | p384 src/ecdsa.rs): the nonce
//            is RFC 6979 (hmac_drbg.hpp) over h1 = Reduce::reduce_bytes of the field-sized prehash (bits2octets) and the canonical key,
//            on the curve's digest (SHA-256; P-384: SHA-384), with NB bytes of additional data in the randomized forms.
//            rfc6979_nonce_kernel -> the unchanged signing pipeline (ecdsa_kernels.hpp).
//   BIP340 - SigningKey::sign_prehash_with_aux_rand (k256/src/schnorr/signing.rs:79-120):
//            P = d G -> schnorr_nonce_kernel: d' = d or n - d by the parity of y(P), t = d' ^ H_aux(aux), rand = H_nonce(t || x(P) || m),
//            k = rand accepted in [1, n - 1] (NonZeroScalar::try_from REJECTS a rand outside: no reduction mod n) -> R = k G ->
//            schnorr_finish_kernel: k negated if y(R) is odd, e = challenge mod n, s = k + e d'.
// Both multiplications run on the constant-time fixed-base kernel.  No branch and no address here depends on a key, a nonce or a value
// derived from them (the DRBG's rejection loop excepted: hmac_drbg.hpp); an invalid key is a mask.  d' and t live in registers only; k
// passes through the intermediate workspace, which the launchers clear (curve_ops.hpp).
// The per-element functions are ECGPU_HD: tests/hosttwin/hosttwin_signing.cpp compiles them for the host.
#pragma once
#include "hmac_drbg.hpp"
#include "h2c_hash.hpp"
#include "scalar_ops.hpp"

namespace ecgpu {
namespace sign {

// NonZeroScalar::try_from: 0 < x < n keeps x and returns 1; anything else clears x and returns 0
template <class O>
ECGPU_HD u32 nonzero_scalar(u32* x) {
  const u32 ok = scops::canon<O>(x);
  return ok & (mp_is_zero<O::L>(x) ? 0u : 1u);
}

// The nonce of one ECDSA signature.  d: the key, z: the field-sized prehash, extra: the additional data (read with EXTRA only), all
// O::L little-endian limbs.  k = 0 for a key outside [1, n - 1] (the generator then runs on x = 0 and its output is masked away).
// Returns the number of rejected candidates.
template <class H, class O, bool EXTRA>
ECGPU_HD int ecdsa_nonce(u32* k, const u32* d, const u32* z, const u32* extra) {
  constexpr int L = O::L;
  u32 x[L], h1[L], q[L], zero[L];
  mp_copy<L>(x, d);
  const u32 ok = nonzero_scalar<O>(x);
  mp_copy<L>(h1, z);
  smont::reduce_once<O>(h1);                       // the prehash is below 2^(32 L) < 2n
  smont::order<O>(q);
  const int rejected = rfc6979::generate_k<H, L, EXTRA>(k, x, h1, extra, q);
  mp_zero<L>(zero);
  mp_select<L>(k, ok != 0, k, zero);
  return rejected;
}

// the states after the block t || t, t = SHA256(tag) (h2c_hash.hpp has the challenge's)
static constexpr u32 BIP340_AUX_MID[8] = {0x24DD3219u, 0x4EBA7E70u, 0xCA0FABB9u, 0x0FA3166Du, 0x3AFBE4B1u, 0x4C44DF97u, 0x4AAC2739u, 0x249E850Au};
static constexpr u32 BIP340_NONCE_MID[8] = {0x46615B35u, 0xF4BFBFF7u, 0x9F8DC671u, 0x83627AB3u, 0x60217180u, 0x57358661u, 0x21A29E54u, 0x68B07B4Cu};

// SigningKey::from: the key whose public point has an even y.  d in [1, n - 1], limbs.
ECGPU_HD void bip340_even_key(u32* dp, const u32* d, u32 p_y_odd) {
  u32 nd[8];
  smont::neg<K256Order>(nd, d);
  mp_select<8>(dp, p_y_odd != 0, nd, d);
}
// rand = H_nonce((d' ^ H_aux(aux)) || x(P) || m) as limbs.  px, aux, m: 8 words each as they lie in memory.
ECGPU_HD void bip340_nonce_hash(u32* rand, const u32* dp, const u32* px, const u32* aux, const u32* m) {
  using H = sha2::Sha256;
  u32 h[8], w[16];
#pragma unroll
  for (int i = 0; i < 8; i++) { h[i] = BIP340_AUX_MID[i]; w[i] = bswap32(aux[i]); w[8 + i] = 0; }
  w[8] = 0x80000000u;
  w[15] = (64 + 32) * 8;
  sha2::compress<H>(h, w);
#pragma unroll
  for (int i = 0; i < 8; i++) { w[i] = dp[7 - i] ^ h[i]; w[8 + i] = bswap32(px[i]); h[i] = BIP340_NONCE_MID[i]; }     // t || x(P)
  sha2::compress<H>(h, w);
#pragma unroll
  for (int i = 0; i < 8; i++) { w[i] = bswap32(m[i]); w[8 + i] = 0; }
  w[8] = 0x80000000u;
  w[15] = (64 + 96) * 8;
  sha2::compress<H>(h, w);
#pragma unroll
  for (int i = 0; i < 8; i++) rand[i] = h[7 - i];
}
// s = k' + e d' with k' = k or n - k by the parity of y(R) and e = challenge(r, x(P), m) mod n.  k, dp in [0, n - 1] as limbs;
// r, px, m: 8 words each as they lie in memory.  Returns 1 and s, or 0 and s = 0 where s is zero (the reference returns Err).
ECGPU_HD u32 bip340_finish(u32* s, const u32* k, u32 r_y_odd, const u32* dp, const u32* r, const u32* px, const u32* m) {
  using O = K256Order;
  u32 kk[8], nk[8], e_be[8], e[8], ed[8];
  smont::neg<O>(nk, k);
  mp_select<8>(kk, r_y_odd != 0, nk, k);
  h2c::bip340_challenge(e_be, r, px, m);
  words_load_be<8>(e, e_be);
  smont::reduce_once<O>(e);
  scops::mul_plain<O>(ed, e, dp);
  smont::add<O>(s, kk, ed);
  return mp_is_zero<8>(s) ? 0u : 1u;
}

}  // namespace sign
}  // namespace ecgpu

#if defined(__HIPCC__)
#include "ecdsa_kernels.hpp"

namespace ecgpu {
namespace sign {

// out_k[i] = the RFC 6979 nonce of (d[i], z[i] [, extra[i]]), 0 for a key outside [1, n - 1]; one signature per lane
template <class C, bool EXTRA>
__global__ void __launch_bounds__(256) rfc6979_nonce_kernel(const u32* d, const u32* z, const u32* extra, u32* out_k, size_t n) {
  using O = OrderOf<C>;
  using H = typename h2c::Suite<C>::Hash;
  constexpr int L = O::L;
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) {
    u32 dd[L], zz[L], ee[L], k[L];
    words_load_be<L>(dd, d + i * L);
    words_load_be<L>(zz, z + i * L);
    if constexpr (EXTRA) words_load_be<L>(ee, extra + i * L);
    else mp_zero<L>(ee);
    (void)ecdsa_nonce<H, O, EXTRA>(k, dd, zz, ee);
    words_store_be<L>(out_k + i * L, k);
  }
}

// k[i] = the accepted BIP340 nonce of (d[i], aux[i], m[i]) under P[i] = d[i] G (p_xy, affine), 0 where the key or rand is outside [1, n - 1]
template <int UNUSED>      // a template only so that the header can be included by every curve's translation unit
__global__ void __launch_bounds__(256) schnorr_nonce_kernel(const u32* d, const u32* p_xy, const u32* aux, const u32* m, u32* k, size_t n) {
  using O = K256Order;
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) {
    u32 dd[8], dp[8], rand[8], zero[8];
    words_load_be<8>(dd, d + i * 8);
    u32 ok = nonzero_scalar<O>(dd);
    bip340_even_key(dp, dd, bswap32(p_xy[i * 16 + 15]) & 1u);
    bip340_nonce_hash(rand, dp, p_xy + i * 16, aux + i * 8, m + i * 8);
    ok &= nonzero_scalar<O>(rand);
    mp_zero<8>(zero);
    mp_select<8>(rand, ok != 0, rand, zero);
    words_store_be<8>(k + i * 8, rand);
  }
}
// sig[i] = x(R) || s, pubkeys_x[i] = x(P) (optional), ok[i]; zeros and ok = 0 for a key outside [1, n - 1], a rejected nonce (k = 0) and s = 0
template <int UNUSED>
__global__ void __launch_bounds__(256) schnorr_finish_kernel(const u32* d, const u32* p_xy, const u32* k, const u32* r_xy, const u32* m, u32* sig,
                                                             u32* pubkeys_x, uint8_t* ok, size_t n) {
  using O = K256Order;
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) {
    u32 dd[8], dp[8], kk[8], s[8], s_be[8];
    words_load_be<8>(dd, d + i * 8);
    words_load_be<8>(kk, k + i * 8);
    u32 g = nonzero_scalar<O>(dd) & nonzero_scalar<O>(kk);
    bip340_even_key(dp, dd, bswap32(p_xy[i * 16 + 15]) & 1u);
    g &= bip340_finish(s, kk, bswap32(r_xy[i * 16 + 15]) & 1u, dp, r_xy + i * 16, p_xy + i * 16, m + i * 8);
    words_store_be<8>(s_be, s);
    const u32 mk = 0u - g;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      sig[i * 16 + j] = r_xy[i * 16 + j] & mk;
      sig[i * 16 + 8 + j] = s_be[j] & mk;
      if (pubkeys_x) pubkeys_x[i * 8 + j] = p_xy[i * 16 + j] & mk;
    }
    ok[i] = (uint8_t)g;
  }
}

}  // namespace sign
}  // namespace ecgpu
#endif
