// HMAC (RFC 2104) over sha2.hpp and the deterministic nonce of RFC 6979 section 3.2 (HMAC-DRBG), one signature per lane: what
// SigningKey::sign_prehash of the external ecdsa crate derives before it enters hazmat::sign_prehashed (exercised by the `rfc6979` and
// `prehash_signer_signing_with_*` tests of p256/src/ecdsa.rs and p384/src/ecdsa.rs).
//
// Only what RFC 6979 needs on the three curves: the key of an HMAC is exactly one digest long (hlen = qlen: SHA-256 with secp256k1
// and P-256, SHA-384 with P-384), so a candidate T is one V and bits2int is the identity.  Every message has a layout known at compile
// time - V || 0x00 || x || h1 is 97 bytes behind the ipad block with SHA-256 - so all of them are built by sha2::place_word /
// place_byte at literal positions: registers only, no byte loader.  A key's ipad and opad midstates are kept for both of its uses
// (K = HMAC(K, ..) and V = HMAC(K, V)).
//
// Constant time: no branch and no address depends on x, K, V or k - with ONE exception, the rejection loop that RFC 6979 prescribes
// (step h.3): a candidate outside [1, q - 1] is dropped and the generator runs on.  That leaks only THAT a candidate was rejected,
// which happens with probability 2^-32 on P-256, 2^-128 on secp256k1 and 2^-194 on P-384.
//
// Compressions per nonce without a rejection: 18 - two per key for three keys, three per K update, two per V update - and 20 on
// SHA-256 with additional data, whose 129-byte seed message takes a third block.
// Everything is ECGPU_HD: tests/hosttwin/hosttwin_signing.cpp compiles the same text for the host.
#pragma once
#include "sha2.hpp"

namespace ecgpu {
namespace hmac {

template <class H> constexpr int digest_words() { return H::DIGEST_BYTES / (int)sizeof(typename H::W); }

// the states after the ipad and the opad block of a key
template <class H>
struct Key {
  typename H::W inner[8], outer[8];
};
// k: the key as digest_words big-endian word values
template <class H>
ECGPU_HD void key_set(Key<H>& key, const typename H::W* k) {
  using W = typename H::W;
  constexpr int DW = digest_words<H>();
  constexpr W IPAD = (W)0x3636363636363636ull, OPAD = (W)0x5C5C5C5C5C5C5C5Cull;
  W w[16];
#pragma unroll
  for (int j = 0; j < 16; j++) w[j] = (j < DW ? k[j] : (W)0) ^ IPAD;
#pragma unroll
  for (int i = 0; i < 8; i++) key.inner[i] = H::IV[i];
  sha2::compress<H>(key.inner, w);
#pragma unroll
  for (int j = 0; j < 16; j++) w[j] = (j < DW ? k[j] : (W)0) ^ OPAD;
#pragma unroll
  for (int i = 0; i < 8; i++) key.outer[i] = H::IV[i];
  sha2::compress<H>(key.outer, w);
}
// the outer hash: out (digest_words words) = H(opad block || inner digest h)
template <class H>
ECGPU_HD void mac_outer(typename H::W* out, const Key<H>& key, const typename H::W* inner) {
  using W = typename H::W;
  constexpr int DW = digest_words<H>();
  W h[8], w[16];
#pragma unroll
  for (int j = 0; j < 16; j++) w[j] = j < DW ? inner[j] : (W)0;
  sha2::pad_message<H>(w, H::DIGEST_BYTES, 1);
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = key.outer[i];
  sha2::compress<H>(h, w);
#pragma unroll
  for (int j = 0; j < DW; j++) out[j] = h[j];
}
// out = HMAC(key, message).  m: the message of MSG_BYTES bytes as placed words with zeros behind, in sha2::padded_blocks(MSG_BYTES)
// blocks; it is used up.  out may be the key's own source or a part of the message's.
template <class H, u32 MSG_BYTES>
ECGPU_HD void mac(typename H::W* out, const Key<H>& key, typename H::W* m) {
  typename H::W h[8];
  sha2::pad_message<H>(m, MSG_BYTES, 1);
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = key.inner[i];
#pragma unroll
  for (u32 b = 0; b < sha2::padded_blocks<H>(MSG_BYTES); b++) sha2::compress<H>(h, m + 16 * b);
  mac_outer<H>(out, key, h);
}
// the same for a length known only at run time (the host twin's test of the pieces above; no kernel calls it)
template <class H>
ECGPU_HD void mac_any(typename H::W* out, const Key<H>& key, typename H::W* m, u32 msg_bytes) {
  typename H::W h[8];
  sha2::pad_message<H>(m, msg_bytes, 1);
  for (int i = 0; i < 8; i++) h[i] = key.inner[i];
  for (u32 b = 0; b < sha2::padded_blocks<H>(msg_bytes); b++) sha2::compress<H>(h, m + 16 * b);
  mac_outer<H>(out, key, h);
}

}  // namespace hmac

namespace rfc6979 {

// NW little-endian 32-bit limbs <-> the same integer as big-endian hash words
template <class H, int NW>
ECGPU_HD void to_hash_words(typename H::W* w, const u32* limbs) {
  constexpr int DW = hmac::digest_words<H>();
#pragma unroll
  for (int j = 0; j < DW; j++) {
    if constexpr (sizeof(typename H::W) == 4) w[j] = limbs[NW - 1 - j];
    else w[j] = (u64)limbs[NW - 1 - 2 * j] << 32 | limbs[NW - 2 - 2 * j];
  }
}
template <class H, int NW>
ECGPU_HD void from_hash_words(u32* limbs, const typename H::W* w) {
  constexpr int DW = hmac::digest_words<H>();
#pragma unroll
  for (int j = 0; j < DW; j++) {
    if constexpr (sizeof(typename H::W) == 4) limbs[NW - 1 - j] = (u32)w[j];
    else { limbs[NW - 1 - 2 * j] = (u32)(w[j] >> 32); limbs[NW - 2 - 2 * j] = (u32)w[j]; }
  }
}

// RFC 6979 section 3.2, steps b to h.  x: the key, h1: bits2octets of the digest (already below q), extra: the additional data k' of
// section 3.6 (read only with EXTRA), q: the order - all NW little-endian limbs, NW words being one digest of H.  Writes the nonce
// k, 0 < k < q, and returns how many candidates were rejected on the way.  q is an argument (not the curve's constant) so that the
// host twin can drive the rejection branch with a modulus that rejects often.
//
// One loop runs the whole generator so that every piece of it is instantiated once (each compression is ~1 K instructions):
//   round -1: the key K = 0x00..            round 0, 1: K = HMAC(K, V || round || x || h1 [|| extra]), V = HMAC(K, V)
//   from round 1 on: T = V = HMAC(K, V), accepted if in range; round 2, 3, ..: K = HMAC(K, V || 0x00), V = HMAC(K, V) first
template <class H, int NW, bool EXTRA>
ECGPU_HD int generate_k(u32* k, const u32* x, const u32* h1, const u32* extra, const u32* q) {
  using W = typename H::W;
  constexpr int DW = hmac::digest_words<H>();
  constexpr u32 NB = H::DIGEST_BYTES, WB = sizeof(W);
  static_assert(NW * 4 == (int)NB, "hlen = qlen: one digest is one scalar");
  constexpr u32 SEED_BYTES = NB + 1 + 2 * NB + (EXTRA ? NB : 0);
  constexpr int SEED_WORDS = 16 * (int)sha2::padded_blocks<H>(SEED_BYTES);
  static_assert(sha2::padded_blocks<H>(NB + 1) == 1, "V || 0x00 and its padding are one block");
  W xs[DW], hs[DW], es[DW], K[DW], V[DW];
  to_hash_words<H, NW>(xs, x);
  to_hash_words<H, NW>(hs, h1);
  if constexpr (EXTRA) to_hash_words<H, NW>(es, extra);
#pragma unroll
  for (int j = 0; j < DW; j++) { K[j] = 0; V[j] = (W)0x0101010101010101ull; }
  hmac::Key<H> key;
  int round = -1;
#pragma unroll 1
  for (;; round++) {
    if (round >= 0 && round < 2) {
      W m[SEED_WORDS];
#pragma unroll
      for (int j = 0; j < SEED_WORDS; j++) m[j] = j < DW ? V[j] : (W)0;
      sha2::place_byte<H>(m, NB, (u32)round);
#pragma unroll
      for (int j = 0; j < DW; j++) {
        sha2::place_word<H>(m, NB + 1 + j * WB, xs[j]);
        sha2::place_word<H>(m, 2 * NB + 1 + j * WB, hs[j]);
        if constexpr (EXTRA) sha2::place_word<H>(m, 3 * NB + 1 + j * WB, es[j]);
      }
      hmac::mac<H, SEED_BYTES>(K, key, m);
    } else if (round >= 2) {
      W m[16];
#pragma unroll
      for (int j = 0; j < 16; j++) m[j] = j < DW ? V[j] : (W)0;          // V || 0x00: the separator byte is the zero behind V
      hmac::mac<H, NB + 1>(K, key, m);
    }
    hmac::key_set<H>(key, K);
    if (round < 0) continue;
    // V = HMAC(K, V); from round 1 on once more for the candidate
#pragma unroll 1
    for (int u = 0; u < (round >= 1 ? 2 : 1); u++) {
      W m[16];
#pragma unroll
      for (int j = 0; j < 16; j++) m[j] = j < DW ? V[j] : (W)0;
      hmac::mac<H, NB>(V, key, m);
    }
    if (round < 1) continue;
    from_hash_words<H, NW>(k, V);
    if (!mp_is_zero<NW>(k) && !mp_geq<NW>(k, q)) break;                  // the one secret-dependent branch: RFC 6979 step h.3
  }
  return round - 1;
}

}  // namespace rfc6979
}  // namespace ecgpu
