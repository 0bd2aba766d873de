// TEST-ONLY host build of deterministic signing (sha2.hpp word placement, hmac_drbg.hpp, signing_kernels.hpp): HMAC, the RFC 6979
// generator, the BIP340 tag midstates and the nonce, accept and finish steps.  Checked against hmac / hashlib, tests/rfc6979_model.py
// and the oracle by tests/test_hosttwin_signing.py.
#include <string.h>
#include <vector>
#include "hosttwin_trace.hpp"
#include "signing_kernels.hpp"
using namespace ecgpu;

// big-endian bytes <-> NW little-endian limbs
template <int NW>
static void limbs_from(u32* limbs, const uint8_t* p) {
  u32 be[NW];
  memcpy(be, p, 4 * NW);
  words_load_be<NW>(limbs, be);
}
template <int NW>
static void limbs_to(uint8_t* p, const u32* limbs) {
  u32 be[NW];
  words_store_be<NW>(be, limbs);
  memcpy(p, be, 4 * NW);
}

// HMAC of a message of any length over the code the generator uses: the message goes into the word array by place_byte (its first
// len mod W bytes) and then by place_word at the byte positions that leaves - every alignment of a word in its two slots -, the
// key's two midstates come from key_set, padding, compressions and the outer hash from mac_any (mac with a run-time length).
template <class H>
static int hmac_bytes(const uint8_t* key, const uint8_t* msg, size_t len, uint8_t* out) {
  using W = typename H::W;
  constexpr int DW = hmac::digest_words<H>();
  constexpr size_t WB = sizeof(W);
  W kw[DW], d[DW];
  for (int j = 0; j < DW; j++) {
    kw[j] = 0;
    for (size_t b = 0; b < WB; b++) kw[j] = kw[j] << 8 | key[j * WB + b];
  }
  hmac::Key<H> k;
  hmac::key_set<H>(k, kw);
  std::vector<W> m(16 * sha2::padded_blocks<H>((u32)len), 0);
  size_t pos = 0;
  for (; pos < len % WB; pos++) sha2::place_byte<H>(m.data(), (u32)pos, msg[pos]);
  for (; pos < len; pos += WB) {
    W w = 0;
    for (size_t b = 0; b < WB; b++) w = w << 8 | msg[pos + b];
    sha2::place_word<H>(m.data(), (u32)pos, w);
  }
  hmac::mac_any<H>(d, k, m.data(), (u32)len);
  for (int j = 0; j < DW; j++)
    for (size_t b = 0; b < WB; b++) out[j * WB + b] = (uint8_t)(d[j] >> (8 * (WB - 1 - b)));
  return 0;
}

template <class H, int NW>
static int gen_k(const uint8_t* x, const uint8_t* h1, const uint8_t* extra, const uint8_t* q, uint8_t* k) {
  u32 xl[NW], hl[NW], el[NW], ql[NW], kl[NW];
  limbs_from<NW>(xl, x);
  limbs_from<NW>(hl, h1);
  limbs_from<NW>(ql, q);
  int rejected;
  if (extra) {
    limbs_from<NW>(el, extra);
    rejected = rfc6979::generate_k<H, NW, true>(kl, xl, hl, el, ql);
  } else {
    rejected = rfc6979::generate_k<H, NW, false>(kl, xl, hl, nullptr, ql);
  }
  limbs_to<NW>(k, kl);
  return rejected;
}
template <class H, class O>
static int nonce(const uint8_t* d, const uint8_t* z, const uint8_t* extra, uint8_t* k) {
  constexpr int L = O::L;
  u32 dl[L], zl[L], el[L], kl[L];
  limbs_from<L>(dl, d);
  limbs_from<L>(zl, z);
  int rejected;
  if (extra) {
    limbs_from<L>(el, extra);
    rejected = sign::ecdsa_nonce<H, O, true>(kl, dl, zl, el);
  } else {
    rejected = sign::ecdsa_nonce<H, O, false>(kl, dl, zl, nullptr);
  }
  limbs_to<L>(k, kl);
  return rejected;
}

extern "C" {
// hash: 0 SHA-256, 1 SHA-384; key: one digest long
int ht_hmac(int hash, const uint8_t* key, const uint8_t* msg, size_t len, uint8_t* out) {
  if (hash == 0) return hmac_bytes<sha2::Sha256>(key, msg, len, out);
  if (hash == 1) return hmac_bytes<sha2::Sha384>(key, msg, len, out);
  return -1;
}
// rfc6979::generate_k with an order of the caller's choice: x, h1, extra (or NULL), q, k of one digest each; returns the rejections
int ht_rfc6979_generate_k(int hash, const uint8_t* x, const uint8_t* h1, const uint8_t* extra, const uint8_t* q, uint8_t* k) {
  if (hash == 0) return gen_k<sha2::Sha256, 8>(x, h1, extra, q, k);
  if (hash == 1) return gen_k<sha2::Sha384, 12>(x, h1, extra, q, k);
  return -1;
}
// the nonce of one ECDSA signature as the kernel derives it: key d, field-sized prehash z, extra or NULL; returns the rejections
int ht_ecdsa_nonce(int curve, const uint8_t* d, const uint8_t* z, const uint8_t* extra, uint8_t* k) {
  if (curve == 0) return nonce<sha2::Sha256, K256Order>(d, z, extra, k);
  if (curve == 1) return nonce<sha2::Sha256, P256Order>(d, z, extra, k);
  if (curve == 2) return nonce<sha2::Sha384, P384Order>(d, z, extra, k);
  return -1;
}
// the digest a hash started from a tag midstate gives for an empty remainder: SHA256(t || t); which: 0 challenge, 1 aux, 2 nonce
int ht_bip340_midstate_digest(int which, uint8_t* out) {
  const u32* mid = which == 0 ? h2c::BIP340_CHALLENGE_MID : which == 1 ? sign::BIP340_AUX_MID : which == 2 ? sign::BIP340_NONCE_MID : nullptr;
  if (!mid) return -1;
  sha2::State<sha2::Sha256> s;
  sha2::init_mid<sha2::Sha256>(s, mid, 1);
  u32 d[8];
  sha2::finish(s, d);
  for (int i = 0; i < 32; i++) out[i] = (uint8_t)sha2::digest_byte<sha2::Sha256>(d, (u32)i);
  return 0;
}
// d' and rand of one signature: key d in [1, n - 1], parity of y(P), x(P), aux, m (32 bytes each)
int ht_bip340_nonce(const uint8_t* d, int p_y_odd, const uint8_t* px, const uint8_t* aux, const uint8_t* m, uint8_t* dprime, uint8_t* rand) {
  u32 dl[8], dp[8], rl[8], pw[8], aw[8], mw[8];
  limbs_from<8>(dl, d);
  memcpy(pw, px, 32); memcpy(aw, aux, 32); memcpy(mw, m, 32);
  sign::bip340_even_key(dp, dl, (u32)p_y_odd);
  sign::bip340_nonce_hash(rl, dp, pw, aw, mw);
  limbs_to<8>(dprime, dp);
  limbs_to<8>(rand, rl);
  return 0;
}
// the accept step (NonZeroScalar::try_from) on the order of `curve`: returns ok; x is cleared where it is refused
int ht_nonzero_scalar(int curve, uint8_t* x) {
  if (curve == 2) {
    u32 l[12];
    limbs_from<12>(l, x);
    const int ok = (int)sign::nonzero_scalar<P384Order>(l);
    limbs_to<12>(x, l);
    return ok;
  }
  u32 l[8];
  limbs_from<8>(l, x);
  const int ok = curve == 0 ? (int)sign::nonzero_scalar<K256Order>(l) : (int)sign::nonzero_scalar<P256Order>(l);
  limbs_to<8>(x, l);
  return ok;
}
// the finish step: k, d' in [0, n - 1], parity of y(R), r = x(R), x(P), m; returns ok and writes s
int ht_bip340_finish(const uint8_t* k, int r_y_odd, const uint8_t* dprime, const uint8_t* r, const uint8_t* px, const uint8_t* m, uint8_t* s) {
  u32 kl[8], dp[8], sl[8], rw[8], pw[8], mw[8];
  limbs_from<8>(kl, k);
  limbs_from<8>(dp, dprime);
  memcpy(rw, r, 32); memcpy(pw, px, 32); memcpy(mw, m, 32);
  const int ok = (int)sign::bip340_finish(sl, kl, (u32)r_y_odd, dp, rw, pw, mw);
  limbs_to<8>(s, sl);
  return ok;
}
}
