// TEST-ONLY host build of the sponge digests (keccak.hpp digest_words over update_aligned): whole blocks of a 4-byte aligned record
// by words, everything else by bytes.  Checked against hashlib (SHA-3) and tests/keccak_model.py (Keccak-256) by
// tests/test_hosttwin_keccak.py.
#include <string.h>
#include "keccak.hpp"
using namespace ecgpu;

template <class H>
static int digest_at(const uint8_t* msg, size_t len, uint8_t* out) {
  u32 w[H::DIGEST_BYTES / 4];
  keccak::digest_words<H>(w, msg, (u32)len);
  memcpy(out, w, H::DIGEST_BYTES);
  return 0;
}
// the first `split` bytes through the byte path, the rest through update_aligned: the word path behind a byte-path update
template <class H>
static int digest_split(const uint8_t* msg, size_t len, size_t split, uint8_t* out) {
  if (split > len) return -1;
  keccak::State<H> s;
  keccak::init(s);
  keccak::update(s, msg, (u32)split);
  keccak::update_aligned(s, msg + split, (u32)(len - split));
  keccak::finish(s);
  for (int i = 0; i < H::DIGEST_BYTES; i++) out[i] = (uint8_t)(s.a[i / 8] >> (8 * (i % 8)));
  return 0;
}
static size_t rate_of(int hash) { return hash == 16 || hash == 17 ? 136 : hash == 18 ? 104 : 0; }

extern "C" {
// hash (ecgpu_hash): 16 Keccak-256, 17 SHA3-256 (32 bytes out), 18 SHA3-384 (48 bytes out); the message is the len bytes at base + offset
int ht_keccak(int hash, const uint8_t* base, size_t offset, size_t len, uint8_t* out) {
  if (hash == 16) return digest_at<keccak::Keccak256>(base + offset, len, out);
  if (hash == 17) return digest_at<keccak::Sha3_256>(base + offset, len, out);
  if (hash == 18) return digest_at<keccak::Sha3_384>(base + offset, len, out);
  return -1;
}
int ht_keccak_split(int hash, const uint8_t* base, size_t offset, size_t len, size_t split, uint8_t* out) {
  if (hash == 16) return digest_split<keccak::Keccak256>(base + offset, len, split, out);
  if (hash == 17) return digest_split<keccak::Sha3_256>(base + offset, len, split, out);
  if (hash == 18) return digest_split<keccak::Sha3_384>(base + offset, len, split, out);
  return -1;
}
// 1 if a message of len bytes at base + offset has its whole blocks read by words (the public condition of update_aligned)
int ht_keccak_takes_words(int hash, const uint8_t* base, size_t offset, size_t len) {
  const size_t rate = rate_of(hash);
  if (!rate) return -1;
  return ((uintptr_t)(base + offset) & 3u) == 0 && len >= rate;
}
}
