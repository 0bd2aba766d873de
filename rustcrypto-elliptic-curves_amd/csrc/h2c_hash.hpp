// The byte side of hash to curve (RFC 9380) on the device: expand_message_xmd over sha2.hpp (ExpandMsgXmd of the external
// elliptic-curve crate, as k256 | p256 | p384 src/arithmetic/hash2curve.rs use it), FromOkm for FieldElement (the same files),
// and the BIP340 challenge hash (k256/src/schnorr.rs:180-186, verifying.rs:75-83).  The map itself is h2c_map.hpp.
//
//   b_0 = H(Z_pad || msg || I2OSP(len_in_bytes, 2) || I2OSP(0, 1) || DST')        DST' = DST || I2OSP(len(DST), 1)
//   b_1 = H(b_0 || I2OSP(1, 1) || DST')       b_i = H((b_0 ^ b_(i-1)) || I2OSP(i, 1) || DST')
// Out of scope: a DST above 255 bytes (the RFC's rehash to "H2C-OVERSIZE-DST-" || DST) - the entry points refuse it - and
// expand_message_xof.
//
// Everything but the kernels is ECGPU_HD (tests/hosttwin/hosttwin_h2c_hash.cpp compiles it for the host).
#pragma once
#include "sha2.hpp"
#include "traits.hpp"
#include "xmd_tail.hpp"

namespace ecgpu {
namespace h2c {

// sink(i, d): block b_(i+1) as digest words (big-endian values; the first DIGEST_BYTES / sizeof(W) of d count), i = 0 .. ell - 1.
// ONE loop produces b_0 (pass 0) and the output blocks, so that the compression is instantiated three times, not seven.
template <class H, class Sink>
ECGPU_HD void expand_message_xmd(const uint8_t* msg, u32 msg_len, const XmdTail& tail, Sink&& sink) {
  using W = typename H::W;
  constexpr int DW = H::DIGEST_BYTES / sizeof(W);
  const u32 ell = (tail.out_len + H::DIGEST_BYTES - 1) / H::DIGEST_BYTES;
  W b0[DW], prev[DW];
#pragma unroll
  for (int j = 0; j < DW; j++) { b0[j] = 0; prev[j] = 0; }
#pragma unroll 1
  for (u32 i = 0; i <= ell; i++) {
    sha2::State<H> s;
    if (i == 0) {
      sha2::init_mid<H>(s, H::ZPAD, 1);
      sha2::update(s, msg, msg_len);
    } else {
      W in[DW];
#pragma unroll
      for (int j = 0; j < DW; j++) in[j] = b0[j] ^ prev[j];          // prev = 0 for b_1
      sha2::init_words<H, DW>(s, in);
      sha2::put_byte(s, i);
    }
    sha2::update(s, tail.bytes + (i ? 3 : 0), tail.len - (i ? 3 : 0));
    W d[8];
    sha2::finish(s, d);
    if (i == 0) {
#pragma unroll
      for (int j = 0; j < DW; j++) b0[j] = d[j];
    } else {
#pragma unroll
      for (int j = 0; j < DW; j++) prev[j] = d[j];
      sink(i - 1, d);
    }
  }
}

// the uniform bytes as 32-bit words in reading order, o[0] the most significant: NWORDS words written through static indices only
template <class H, int NWORDS>
struct OkmWords {
  u32 o[NWORDS];
  ECGPU_HD void operator()(u32 i, const typename H::W* d) {
    constexpr int DW32 = H::DIGEST_BYTES / 4;
#pragma unroll
    for (int k = 0; k < NWORDS; k++) {
      u32 v;
      if constexpr (sizeof(typename H::W) == 4) v = (u32)d[k % DW32];
      else v = (k % DW32) & 1 ? (u32)d[(k % DW32) / 2] : (u32)(d[(k % DW32) / 2] >> 32);
      o[k] = ((u32)(k / DW32) == i) ? v : o[k];
    }
  }
};

// The curve's own hash and FromOkm::Length
template <class C> struct Suite {
  using Hash = sha2::Sha256;
  static constexpr int L = 48;
};
template <> struct Suite<CurveP384> {
  using Hash = sha2::Sha384;
  static constexpr int L = 72;
};

// FromOkm for FieldElement: r = okm mod p for the L-byte big-endian okm given as L / 4 words, o[0] the most significant.
// secp256k1: the 12 words are a short 16-word product for the pseudo-Mersenne fold (fe_k256.hpp reduce16).  P-256 / P-384: the
// reference's own d0 2^(4 L) + d1 with both halves below p (L / 2 bytes < NB), in Montgomery form.
template <class C>
ECGPU_HD void field_from_okm(typename C::Fe& r, const u32* o) {
  constexpr int LW = Suite<C>::L / 4;
  if constexpr (C::ID == 0) {
    u32 w[16];
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = k < LW ? o[LW - 1 - k] : 0u;
    k256::reduce16(r, w);
  } else {
    constexpr int NW = C::NW, HW = LW / 2;
    static_assert(HW < NW, "a half of the okm is below p");
    u32 d0[NW], d1[NW], f[NW];
#pragma unroll
    for (int k = 0; k < NW; k++) {
      d1[k] = k < HW ? o[LW - 1 - k] : 0u;
      d0[k] = k < HW ? o[HW - 1 - k] : 0u;
      f[k] = k == HW ? 1u : 0u;                                       // 2^(32 HW) = 2^(4 L)
    }
    typename C::Fe m0, m1, mf;
    mont::to_mont<typename C::Mod>(m0, d0);
    mont::to_mont<typename C::Mod>(m1, d1);
    mont::to_mont<typename C::Mod>(mf, f);
    C::fe_mul(m0, m0, mf);
    C::fe_add(r, m0, m1);
  }
}

// hash_to_field: `count` (1 or 2) field elements of one message, canonical big-endian, into u (count x NW words)
template <class C, int COUNT>
ECGPU_HD void hash_to_field(u32* u, const uint8_t* msg, u32 msg_len, const XmdTail& tail) {
  using H = typename Suite<C>::Hash;
  constexpr int LW = Suite<C>::L / 4, DW32 = H::DIGEST_BYTES / 4;
  constexpr int NWORDS = (COUNT * LW + DW32 - 1) / DW32 * DW32;
  OkmWords<H, NWORDS> okm;
#pragma unroll
  for (int k = 0; k < NWORDS; k++) okm.o[k] = 0;
  expand_message_xmd<H>(msg, msg_len, tail, okm);
#pragma unroll
  for (int e = 0; e < COUNT; e++) {
    typename C::Fe r;
    field_from_okm<C>(r, okm.o + e * LW);
    C::fe_store(u + e * C::NW, r);
  }
}

// e = SHA256(t || t || r || P.x || m), t = SHA256("BIP0340/challenge"): the state after the block t || t is a constant.
// r, px, m, e: 8 words each as they lie in memory (big-endian byte strings read as u32).
static constexpr u32 BIP340_CHALLENGE_MID[8] = {0x9CECBA11u, 0x23925381u, 0x11679112u, 0xD1627E0Fu, 0x97C87550u, 0x003CC765u, 0x90F61164u, 0x33E9B66Au};
ECGPU_HD void bip340_challenge(u32* e, const u32* r, const u32* px, const u32* m) {
  using H = sha2::Sha256;
  u32 h[8], w[16];
#pragma unroll
  for (int i = 0; i < 8; i++) { h[i] = BIP340_CHALLENGE_MID[i]; w[i] = bswap32(r[i]); w[8 + i] = bswap32(px[i]); }
  sha2::compress<H>(h, w);
#pragma unroll
  for (int i = 0; i < 8; i++) { w[i] = bswap32(m[i]); w[8 + i] = 0; }
  w[8] = 0x80000000u;
  w[15] = (64 + 96) * 8;
  sha2::compress<H>(h, w);
#pragma unroll
  for (int i = 0; i < 8; i++) e[i] = bswap32(h[i]);
}

// The plain digest of one message (Digest::digest; what Signer::sign and Verifier::verify of the ecdsa crate and k256's BIP340 keys
// run before their prehash forms) as DIGEST_BYTES / 4 words as they lie in memory: out is 4-byte aligned, so that a prehash
// kernel reads the row as const uint32_t*.  Whole blocks of a 4-byte aligned record come in by words (sha2::update_aligned).
template <class H>
ECGPU_HD void digest_words(u32* out, const uint8_t* msg, u32 msg_len) {
  using W = typename H::W;
  sha2::State<H> s;
  sha2::init(s);
  sha2::update_aligned(s, msg, msg_len);
  W d[8];
  sha2::finish(s, d);
#pragma unroll
  for (int j = 0; j < H::DIGEST_BYTES / (int)sizeof(W); j++) {
    if constexpr (sizeof(W) == 4) out[j] = bswap32(d[j]);
    else { out[2 * j] = bswap32((u32)(d[j] >> 32)); out[2 * j + 1] = bswap32((u32)d[j]); }
  }
}

#if defined(__HIPCC__)
// message i: msg_stride bytes at msgs + i * msg_stride, of which msg_len[i] count (all of them without msg_len).  A length
// above the stride is the caller's error (refused for host buffers); it is clamped so that no read leaves the record.
__device__ __forceinline__ u32 message_length(const u32* msg_len, size_t i, size_t msg_stride) {
  const u32 s = (u32)msg_stride;
  if (!msg_len) return s;
  const u32 l = msg_len[i];
  return l < s ? l : s;
}

// expand_message_xmd to raw bytes: out[i] = tail.out_len uniform bytes
template <class H>
__global__ void __launch_bounds__(256) xmd_kernel(const uint8_t* msgs, size_t msg_stride, const u32* msg_len, const XmdTail tail, uint8_t* out, size_t n) {
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) {
    uint8_t* o = out + i * tail.out_len;
    const u32 out_len = tail.out_len;
    expand_message_xmd<H>(msgs + i * msg_stride, message_length(msg_len, i, msg_stride), tail, [&](u32 blk, const typename H::W* d) {
      const u32 base = blk * H::DIGEST_BYTES;
#pragma unroll 4
      for (u32 k = 0; k < (u32)H::DIGEST_BYTES; k++)
        if (base + k < out_len) o[base + k] = (uint8_t)sha2::digest_byte<H>(d, k);
    });
  }
}
// plain digests: out[i] = the DIGEST_BYTES of message i (rows 4-byte aligned)
template <class H>
__global__ void __launch_bounds__(256) digest_kernel(const uint8_t* msgs, size_t msg_stride, const u32* msg_len, u32* out, size_t n) {
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T)
    digest_words<H>(out + i * (H::DIGEST_BYTES / 4), msgs + i * msg_stride, message_length(msg_len, i, msg_stride));
}
// expand_message_xmd fused with FromOkm: u[i] = count field elements in the layout h2c::map_kernel reads
template <class C, int COUNT>
__global__ void __launch_bounds__(256) hash_to_field_kernel(const uint8_t* msgs, size_t msg_stride, const u32* msg_len, const XmdTail tail, u32* u, size_t n) {
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T)
    hash_to_field<C, COUNT>(u + i * COUNT * C::NW, msgs + i * msg_stride, message_length(msg_len, i, msg_stride), tail);
}
// FromOkm for FieldElement: okm = n records of L bytes (any alignment), out = n canonical field elements
template <class C>
__global__ void __launch_bounds__(256) field_from_okm_kernel(const uint8_t* okm, u32* out, size_t n) {
  constexpr int L = Suite<C>::L, LW = L / 4;
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) {
    const uint8_t* p = okm + i * L;
    u32 o[LW];
#pragma unroll
    for (int k = 0; k < LW; k++) o[k] = (u32)p[4 * k] << 24 | (u32)p[4 * k + 1] << 16 | (u32)p[4 * k + 2] << 8 | (u32)p[4 * k + 3];
    typename C::Fe r;
    field_from_okm<C>(r, o);
    C::fe_store(out + i * C::NW, r);
  }
}
// BIP340 challenges of n signatures: sig = r || s (16 words), px and m 8 words each
template <int UNUSED>      // a template only so that the header can be included by every curve's translation unit
__global__ void __launch_bounds__(256) bip340_challenge_kernel(const u32* px, const u32* sig, const u32* m, u32* e, size_t n) {
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) bip340_challenge(e + i * 8, sig + i * 16, px + i * 8, m + i * 8);
}
#endif

}  // namespace h2c
}  // namespace ecgpu
