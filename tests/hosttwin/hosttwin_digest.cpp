// TEST-ONLY host build of the plain digest (h2c_hash.hpp digest_words over sha2.hpp update_aligned): whole blocks of a 4-byte
// aligned record by words, everything else by bytes.  Checked against hashlib by tests/test_hosttwin_digest.py.
#include <string.h>
#include "h2c_hash.hpp"
using namespace ecgpu;

template <class H>
static int digest_at(const uint8_t* msg, size_t len, uint8_t* out) {
  u32 w[H::DIGEST_BYTES / 4];
  h2c::digest_words<H>(w, msg, (u32)len);
  memcpy(out, w, H::DIGEST_BYTES);
  return 0;
}
// the first `split` bytes through the byte path, the rest through update_aligned: the word path behind a byte-path update
template <class H>
static int digest_split(const uint8_t* msg, size_t len, size_t split, uint8_t* out) {
  if (split > len) return -1;
  typename H::W d[8];
  sha2::State<H> s;
  sha2::init(s);
  sha2::update(s, msg, (u32)split);
  sha2::update_aligned(s, msg + split, (u32)(len - split));
  sha2::finish(s, d);
  for (int i = 0; i < H::DIGEST_BYTES; i++) out[i] = (uint8_t)sha2::digest_byte<H>(d, (u32)i);
  return 0;
}

extern "C" {
// hash: 0 SHA-256 (32 bytes out), 1 SHA-384 (48 bytes out); the message is the len bytes at base + offset
int ht_digest(int hash, const uint8_t* base, size_t offset, size_t len, uint8_t* out) {
  if (hash == 0) return digest_at<sha2::Sha256>(base + offset, len, out);
  if (hash == 1) return digest_at<sha2::Sha384>(base + offset, len, out);
  return -1;
}
int ht_digest_split(int hash, const uint8_t* base, size_t offset, size_t len, size_t split, uint8_t* out) {
  if (hash == 0) return digest_split<sha2::Sha256>(base + offset, len, split, out);
  if (hash == 1) return digest_split<sha2::Sha384>(base + offset, len, split, out);
  return -1;
}
// 1 if a message of len bytes at base + offset has its whole blocks read by words (the public condition of update_aligned)
int ht_digest_takes_words(int hash, const uint8_t* base, size_t offset, size_t len) {
  const size_t bb = hash == 1 ? 128 : 64;
  return ((uintptr_t)(base + offset) & 3u) == 0 && len >= bb;
}
}
