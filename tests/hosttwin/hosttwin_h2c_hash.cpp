// TEST-ONLY host build of the hash layer of hash to curve (sha2.hpp, h2c_hash.hpp): SHA-256 / SHA-384, expand_message_xmd,
// FromOkm for FieldElement and the BIP340 challenge.  Checked against hashlib, the oracle and Python integers by
// tests/test_hosttwin_h2c_hash.py.
#include <string.h>
#include "hosttwin_trace.hpp"
#include "h2c_hash.hpp"
using namespace ecgpu;

template <class H>
static int sha2_bytes(const uint8_t* msg, size_t len, int split, uint8_t* out) {
  typename H::W d[8];
  sha2::State<H> s;
  sha2::init(s);
  // split >= 0: the message in two updates, cut at `split` (the incremental interface across a block boundary)
  const size_t cut = split >= 0 && (size_t)split <= len ? (size_t)split : len;
  sha2::update(s, msg, (u32)cut);
  sha2::update(s, msg + cut, (u32)(len - cut));
  sha2::finish(s, d);
  for (int i = 0; i < H::DIGEST_BYTES; i++) out[i] = (uint8_t)sha2::digest_byte<H>(d, (u32)i);
  return 0;
}
template <class H>
static int xmd_bytes(const uint8_t* msg, size_t msg_len, const uint8_t* dst, size_t dst_len, uint8_t* out, size_t out_len) {
  if (dst_len < 1 || dst_len > 255 || out_len < 1 || out_len > 255u * H::DIGEST_BYTES) return -1;
  h2c::XmdTail tail;
  h2c::xmd_tail_set(tail, dst, dst_len, out_len);
  h2c::expand_message_xmd<H>(msg, (u32)msg_len, tail, [&](u32 blk, const typename H::W* d) {
    for (u32 k = 0; k < (u32)H::DIGEST_BYTES; k++)
      if ((size_t)blk * H::DIGEST_BYTES + k < out_len) out[(size_t)blk * H::DIGEST_BYTES + k] = (uint8_t)sha2::digest_byte<H>(d, k);
  });
  return 0;
}
template <class C>
static void okm_words(u32* o, const uint8_t* p) {
  for (int k = 0; k < h2c::Suite<C>::L / 4; k++) o[k] = (u32)p[4 * k] << 24 | (u32)p[4 * k + 1] << 16 | (u32)p[4 * k + 2] << 8 | (u32)p[4 * k + 3];
}
template <class C>
static int from_okm_rows(const uint8_t* okm, uint8_t* out, int n) {
  constexpr int L = h2c::Suite<C>::L;
  for (int i = 0; i < n; i++) {
    u32 o[L / 4], w[C::NW];
    okm_words<C>(o, okm + (size_t)L * i);
    typename C::Fe r;
    h2c::field_from_okm<C>(r, o);
    C::fe_store(w, r);
    memcpy(out + (size_t)C::NB * i, w, C::NB);
  }
  return 0;
}
template <class C>
static int h2f(const uint8_t* msg, size_t msg_len, const uint8_t* dst, size_t dst_len, int count, uint8_t* out) {
  if (dst_len < 1 || dst_len > 255) return -1;
  h2c::XmdTail tail;
  h2c::xmd_tail_set(tail, dst, dst_len, (size_t)count * h2c::Suite<C>::L);
  u32 u[2 * C::NW];
  if (count == 2) h2c::hash_to_field<C, 2>(u, msg, (u32)msg_len, tail);
  else if (count == 1) h2c::hash_to_field<C, 1>(u, msg, (u32)msg_len, tail);
  else return -1;
  memcpy(out, u, (size_t)count * C::NB);
  return 0;
}

extern "C" {
// hash: 0 SHA-256 (32 bytes out), 1 SHA-384 (48 bytes out)
int ht_sha2(int hash, const uint8_t* msg, size_t len, uint8_t* out) {
  if (hash == 0) return sha2_bytes<sha2::Sha256>(msg, len, -1, out);
  if (hash == 1) return sha2_bytes<sha2::Sha384>(msg, len, -1, out);
  return -1;
}
int ht_sha2_split(int hash, const uint8_t* msg, size_t len, int split, uint8_t* out) {
  if (hash == 0) return sha2_bytes<sha2::Sha256>(msg, len, split, out);
  if (hash == 1) return sha2_bytes<sha2::Sha384>(msg, len, split, out);
  return -1;
}
int ht_expand_xmd(int hash, const uint8_t* msg, size_t msg_len, const uint8_t* dst, size_t dst_len, uint8_t* out, size_t out_len) {
  if (hash == 0) return xmd_bytes<sha2::Sha256>(msg, msg_len, dst, dst_len, out, out_len);
  if (hash == 1) return xmd_bytes<sha2::Sha384>(msg, msg_len, dst, dst_len, out, out_len);
  return -1;
}
// curve: 0 secp256k1, 1 P-256, 2 P-384; okm: n x L bytes (48 / 48 / 72), out: n x NB canonical big-endian bytes
int ht_field_from_okm(int curve, const uint8_t* okm, uint8_t* out, int n) {
  if (curve == 0) return from_okm_rows<CurveK256>(okm, out, n);
  if (curve == 1) return from_okm_rows<CurveP256>(okm, out, n);
  if (curve == 2) return from_okm_rows<CurveP384>(okm, out, n);
  return -1;
}
// the fused path of the device kernel: count (1 | 2) field elements of one message
int ht_hash_to_field(int curve, const uint8_t* msg, size_t msg_len, const uint8_t* dst, size_t dst_len, int count, uint8_t* out) {
  if (curve == 0) return h2f<CurveK256>(msg, msg_len, dst, dst_len, count, out);
  if (curve == 1) return h2f<CurveP256>(msg, msg_len, dst, dst_len, count, out);
  if (curve == 2) return h2f<CurveP384>(msg, msg_len, dst, dst_len, count, out);
  return -1;
}
// r, px, m, e: 32 bytes each
int ht_schnorr_challenge(const uint8_t* r, const uint8_t* px, const uint8_t* m, uint8_t* e) {
  u32 rw[8], pw[8], mw[8], ew[8];
  memcpy(rw, r, 32); memcpy(pw, px, 32); memcpy(mw, m, 32);
  h2c::bip340_challenge(ew, rw, pw, mw);
  memcpy(e, ew, 32);
  return 0;
}
}
