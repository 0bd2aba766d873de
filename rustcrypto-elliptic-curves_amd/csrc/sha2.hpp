// SHA-256 and SHA-384 (FIPS 180-4) for one message per lane: the hash layer under expand_message_xmd (h2c_hash.hpp) and the
// BIP340 challenge.  SHA-384 is the SHA-512 compression with its own initial state, truncated to six words.
//
// Register shape: the eight state words, and ONE 16-word window that is both the block buffer of the incremental interface
// and the rolling message schedule of the compression (round t reads w[t & 15] and then replaces it with the word of round
// t + 16).  Every index into the window is a compile-time constant - a byte is placed by comparing its position with all
// sixteen slots, not by indexing - so the window stays in registers (a runtime-indexed private array would live in scratch).
// Rounds run in groups of sixteen; the round constants are read with the (wave-uniform) group counter.
//
// Constant time in the message: no branch and no address depends on a message byte.  Lengths are public: they steer the
// loops, the padding and the addresses of the byte loads.  So is the address of a message: update_aligned reads the whole blocks
// of a 4-byte aligned message by words (the digest of whole messages, h2c_hash.hpp digest_words; profiles/message_signing.txt).
//
// rotr on 32 bits is one v_alignbit_b32, on 64 bits two of them on the register halves (profiles/h2c_hash_entry_points.txt).
// Everything is ECGPU_HD: tests/hosttwin compiles the same text for the host.
#pragma once
#include "mp32.hpp"

namespace ecgpu {
namespace sha2 {

ECGPU_HD u32 rotr(u32 x, int n) { return (x >> n) | (x << (32 - n)); }
// the low word of (hi : lo) >> n, 0 < n < 32: the shape the compiler turns into v_alignbit_b32
ECGPU_HD u32 funnel(u32 hi, u32 lo, int n) { return (lo >> n) | (hi << (32 - n)); }
// on the halves: a rotation by 32 and more swaps them first (n is a literal at every call; none is a multiple of 32)
ECGPU_HD u64 rotr(u64 x, int n) {
  const u32 lo = (u32)x, hi = (u32)(x >> 32);
  const u32 a = n < 32 ? lo : hi, b = n < 32 ? hi : lo;
  return ((u64)funnel(a, b, n & 31) << 32) | funnel(b, a, n & 31);
}

struct Sha256 {
  using W = u32;
  static constexpr int ROUNDS = 64, BLOCK_BYTES = 64, DIGEST_BYTES = 32, LEN_BYTES = 8;
  static constexpr u32 IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  // the state after one block of zero bytes: Z_pad of expand_message_xmd
  static constexpr u32 ZPAD[8] = {0xDA5698BEu, 0x17B9B469u, 0x62335799u, 0x779FBECAu, 0x8CE5D491u, 0xC0D26243u, 0xBAFEF9EAu, 0x1837A9D8u};
  static constexpr u32 K[64] = {
      0x428A2F98u, 0x71374491u, 0xB5C0FBCFu, 0xE9B5DBA5u, 0x3956C25Bu, 0x59F111F1u, 0x923F82A4u, 0xAB1C5ED5u,
      0xD807AA98u, 0x12835B01u, 0x243185BEu, 0x550C7DC3u, 0x72BE5D74u, 0x80DEB1FEu, 0x9BDC06A7u, 0xC19BF174u,
      0xE49B69C1u, 0xEFBE4786u, 0x0FC19DC6u, 0x240CA1CCu, 0x2DE92C6Fu, 0x4A7484AAu, 0x5CB0A9DCu, 0x76F988DAu,
      0x983E5152u, 0xA831C66Du, 0xB00327C8u, 0xBF597FC7u, 0xC6E00BF3u, 0xD5A79147u, 0x06CA6351u, 0x14292967u,
      0x27B70A85u, 0x2E1B2138u, 0x4D2C6DFCu, 0x53380D13u, 0x650A7354u, 0x766A0ABBu, 0x81C2C92Eu, 0x92722C85u,
      0xA2BFE8A1u, 0xA81A664Bu, 0xC24B8B70u, 0xC76C51A3u, 0xD192E819u, 0xD6990624u, 0xF40E3585u, 0x106AA070u,
      0x19A4C116u, 0x1E376C08u, 0x2748774Cu, 0x34B0BCB5u, 0x391C0CB3u, 0x4ED8AA4Au, 0x5B9CCA4Fu, 0x682E6FF3u,
      0x748F82EEu, 0x78A5636Fu, 0x84C87814u, 0x8CC70208u, 0x90BEFFFAu, 0xA4506CEBu, 0xBEF9A3F7u, 0xC67178F2u};
  static ECGPU_HD u32 S0(u32 x) { return rotr(x, 2) ^ rotr(x, 13) ^ rotr(x, 22); }
  static ECGPU_HD u32 S1(u32 x) { return rotr(x, 6) ^ rotr(x, 11) ^ rotr(x, 25); }
  static ECGPU_HD u32 s0(u32 x) { return rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3); }
  static ECGPU_HD u32 s1(u32 x) { return rotr(x, 17) ^ rotr(x, 19) ^ (x >> 10); }
};

struct Sha384 {
  using W = u64;
  static constexpr int ROUNDS = 80, BLOCK_BYTES = 128, DIGEST_BYTES = 48, LEN_BYTES = 16;
  static constexpr u64 IV[8] = {0xCBBB9D5DC1059ED8ull, 0x629A292A367CD507ull, 0x9159015A3070DD17ull, 0x152FECD8F70E5939ull,
                                0x67332667FFC00B31ull, 0x8EB44A8768581511ull, 0xDB0C2E0D64F98FA7ull, 0x47B5481DBEFA4FA4ull};
  static constexpr u64 ZPAD[8] = {0x443D3F698FB0CF23ull, 0x80A591795CD757AEull, 0x4A9600972C395335ull, 0x98E763D795C489F7ull,
                                  0xF765EA4B8193F748ull, 0x450E49EC00BC838Cull, 0x871CC1D60F1E68C5ull, 0x943BBF4C8EA94259ull};
  static constexpr u64 K[80] = {
      0x428A2F98D728AE22ull, 0x7137449123EF65CDull, 0xB5C0FBCFEC4D3B2Full, 0xE9B5DBA58189DBBCull,
      0x3956C25BF348B538ull, 0x59F111F1B605D019ull, 0x923F82A4AF194F9Bull, 0xAB1C5ED5DA6D8118ull,
      0xD807AA98A3030242ull, 0x12835B0145706FBEull, 0x243185BE4EE4B28Cull, 0x550C7DC3D5FFB4E2ull,
      0x72BE5D74F27B896Full, 0x80DEB1FE3B1696B1ull, 0x9BDC06A725C71235ull, 0xC19BF174CF692694ull,
      0xE49B69C19EF14AD2ull, 0xEFBE4786384F25E3ull, 0x0FC19DC68B8CD5B5ull, 0x240CA1CC77AC9C65ull,
      0x2DE92C6F592B0275ull, 0x4A7484AA6EA6E483ull, 0x5CB0A9DCBD41FBD4ull, 0x76F988DA831153B5ull,
      0x983E5152EE66DFABull, 0xA831C66D2DB43210ull, 0xB00327C898FB213Full, 0xBF597FC7BEEF0EE4ull,
      0xC6E00BF33DA88FC2ull, 0xD5A79147930AA725ull, 0x06CA6351E003826Full, 0x142929670A0E6E70ull,
      0x27B70A8546D22FFCull, 0x2E1B21385C26C926ull, 0x4D2C6DFC5AC42AEDull, 0x53380D139D95B3DFull,
      0x650A73548BAF63DEull, 0x766A0ABB3C77B2A8ull, 0x81C2C92E47EDAEE6ull, 0x92722C851482353Bull,
      0xA2BFE8A14CF10364ull, 0xA81A664BBC423001ull, 0xC24B8B70D0F89791ull, 0xC76C51A30654BE30ull,
      0xD192E819D6EF5218ull, 0xD69906245565A910ull, 0xF40E35855771202Aull, 0x106AA07032BBD1B8ull,
      0x19A4C116B8D2D0C8ull, 0x1E376C085141AB53ull, 0x2748774CDF8EEB99ull, 0x34B0BCB5E19B48A8ull,
      0x391C0CB3C5C95A63ull, 0x4ED8AA4AE3418ACBull, 0x5B9CCA4F7763E373ull, 0x682E6FF3D6B2B8A3ull,
      0x748F82EE5DEFB2FCull, 0x78A5636F43172F60ull, 0x84C87814A1F0AB72ull, 0x8CC702081A6439ECull,
      0x90BEFFFA23631E28ull, 0xA4506CEBDE82BDE9ull, 0xBEF9A3F7B2C67915ull, 0xC67178F2E372532Bull,
      0xCA273ECEEA26619Cull, 0xD186B8C721C0C207ull, 0xEADA7DD6CDE0EB1Eull, 0xF57D4F7FEE6ED178ull,
      0x06F067AA72176FBAull, 0x0A637DC5A2C898A6ull, 0x113F9804BEF90DAEull, 0x1B710B35131C471Bull,
      0x28DB77F523047D84ull, 0x32CAAB7B40C72493ull, 0x3C9EBE0A15C9BEBCull, 0x431D67C49C100D4Cull,
      0x4CC5D4BECB3E42B6ull, 0x597F299CFC657E2Aull, 0x5FCB6FAB3AD6FAECull, 0x6C44198C4A475817ull};
  static ECGPU_HD u64 S0(u64 x) { return rotr(x, 28) ^ rotr(x, 34) ^ rotr(x, 39); }
  static ECGPU_HD u64 S1(u64 x) { return rotr(x, 14) ^ rotr(x, 18) ^ rotr(x, 41); }
  static ECGPU_HD u64 s0(u64 x) { return rotr(x, 1) ^ rotr(x, 8) ^ (x >> 7); }
  static ECGPU_HD u64 s1(u64 x) { return rotr(x, 19) ^ rotr(x, 61) ^ (x >> 6); }
};

// h += compression of the block in w (sixteen big-endian words).  w is the rolling schedule: its contents are used up.
template <class H>
ECGPU_HD void compress(typename H::W* h, typename H::W* w) {
  using W = typename H::W;
  static_assert(H::ROUNDS % 16 == 0, "rounds run in groups of sixteen");
  W s[8];
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = h[i];
#pragma unroll 1
  for (int t = 0; t < H::ROUNDS; t += 16) {
#pragma unroll
    for (int j = 0; j < 16; j++) {
      // the working variables rotate through s[] by name: round j keeps `a` in s[(8 - j) & 7]
      W &a = s[(0 - j) & 7], &b = s[(1 - j) & 7], &c = s[(2 - j) & 7], &d = s[(3 - j) & 7];
      W &e = s[(4 - j) & 7], &f = s[(5 - j) & 7], &g = s[(6 - j) & 7], &hh = s[(7 - j) & 7];
      const W t1 = hh + H::S1(e) + (g ^ (e & (f ^ g))) + H::K[t + j] + w[j];
      const W t2 = H::S0(a) + ((a & b) | (c & (a | b)));
      d += t1;
      hh = t1 + t2;
    }
    if (t + 16 < H::ROUNDS) {
      // in place and in order: slot j + 14 holds the new word for j >= 2 and still the old one for j < 2, either way W[t + j + 14]
#pragma unroll
      for (int j = 0; j < 16; j++) w[j] += H::s0(w[(j + 1) & 15]) + w[(j + 9) & 15] + H::s1(w[(j + 14) & 15]);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] += s[i];
}

// Incremental hashing.  w holds the bytes of the unfinished block, big-endian in its words, and ZEROS behind them.
template <class H>
struct State {
  typename H::W h[8];
  typename H::W w[16];
  u32 total;              // bytes taken so far (public)
};

template <class H>
ECGPU_HD void clear_block(State<H>& s) {
#pragma unroll
  for (int j = 0; j < 16; j++) s.w[j] = 0;
}
template <class H>
ECGPU_HD void init(State<H>& s) {
#pragma unroll
  for (int i = 0; i < 8; i++) s.h[i] = H::IV[i];
  clear_block(s);
  s.total = 0;
}
// a state that has already taken `blocks` whole blocks and stands at `mid` (a precomputed midstate)
template <class H>
ECGPU_HD void init_mid(State<H>& s, const typename H::W* mid, u32 blocks) {
#pragma unroll
  for (int i = 0; i < 8; i++) s.h[i] = mid[i];
  clear_block(s);
  s.total = blocks * H::BLOCK_BYTES;
}
// a fresh state whose block starts with NW whole words (big-endian word values, e.g. an earlier digest)
template <class H, int NW>
ECGPU_HD void init_words(State<H>& s, const typename H::W* words) {
  static_assert(NW < 16, "the words must leave the block unfinished");
  init(s);
#pragma unroll
  for (int j = 0; j < NW; j++) s.w[j] = words[j];
  s.total = NW * sizeof(typename H::W);
}

// takes len bytes at p (any alignment).  One pass per block: every byte position of the block that lies in
// [fill, fill + take) gets its byte; positions outside read p[off] (a byte that exists) and discard it, so the loads need no
// branch and stay in bounds.
template <class H>
ECGPU_HD void update(State<H>& s, const uint8_t* p, u32 len) {
  using W = typename H::W;
  constexpr u32 BB = H::BLOCK_BYTES, WB = sizeof(W);
  u32 fill = s.total & (BB - 1);
  s.total += len;
  u32 off = 0;
#pragma unroll 1
  while (off < len) {
    const u32 room = BB - fill, left = len - off;
    const u32 take = left < room ? left : room;
#pragma unroll
    for (u32 j = 0; j < 16; j++) {
      W acc = s.w[j];
#pragma unroll
      for (u32 k = 0; k < WB; k++) {
        const u32 rel = j * WB + k - fill;               // wraps for positions before `fill`: then rel >= take
        const bool in = rel < take;
        const u32 v = p[off + (in ? rel : 0u)];
        acc |= (W)(in ? v : 0u) << (8 * (WB - 1 - k));
      }
      s.w[j] = acc;
    }
    off += take;
    fill += take;
    if (fill == BB) {
      compress<H>(s.h, s.w);
      clear_block(s);
      fill = 0;
    }
  }
}
// one naturally aligned 32-bit load, as the big-endian word its four bytes spell
ECGPU_HD u32 load_be32(const uint8_t* p) {
  u32 v;
  __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
  return bswap32(v);
}
// `update` for whole messages: where the state stands at a block boundary and p is 4-byte aligned, every whole block comes in by
// sixteen (SHA-384: thirty-two) aligned 32-bit loads and a byte swap instead of one load and sixteen compares per byte; the
// partial last block, and everything where either condition fails, goes through `update` as it stands.  Which way a message goes
// depends on its address and on lengths alone (public); the word loads lie inside [p, p + len) and round no address.
template <class H>
ECGPU_HD void update_aligned(State<H>& s, const uint8_t* p, u32 len) {
  using W = typename H::W;
  constexpr u32 BB = H::BLOCK_BYTES;
  const bool words = (s.total & (BB - 1)) == 0 && ((uintptr_t)p & 3u) == 0;
  const u32 whole = words ? len / BB : 0u;
#pragma unroll 1
  for (u32 b = 0; b < whole; b++) {
    const uint8_t* q = p + b * BB;
#pragma unroll
    for (u32 j = 0; j < 16; j++) {
      if constexpr (sizeof(W) == 4) s.w[j] = load_be32(q + 4 * j);
      else s.w[j] = (W)load_be32(q + 8 * j) << 32 | load_be32(q + 8 * j + 4);
    }
    compress<H>(s.h, s.w);
  }
  if (whole) clear_block(s);
  s.total += whole * BB;
  update(s, p + whole * BB, len - whole * BB);
}
// one byte whose position does not end the block (the caller knows the fill: a counter behind a digest)
template <class H>
ECGPU_HD void put_byte(State<H>& s, u32 byte) {
  using W = typename H::W;
  constexpr u32 BB = H::BLOCK_BYTES, WB = sizeof(W);
  const u32 fill = s.total & (BB - 1);
#pragma unroll
  for (u32 j = 0; j < 16; j++) s.w[j] |= (fill / WB == j) ? (W)byte << (8 * (WB - 1 - fill % WB)) : (W)0;
  s.total += 1;
}
// padding and length; out: the eight state words (the digest is the first DIGEST_BYTES bytes of their big-endian form)
template <class H>
ECGPU_HD void finish(State<H>& s, typename H::W* out) {
  using W = typename H::W;
  constexpr u32 BB = H::BLOCK_BYTES, WB = sizeof(W);
  const u32 fill = s.total & (BB - 1);
#pragma unroll
  for (u32 j = 0; j < 16; j++) s.w[j] |= (fill / WB == j) ? (W)0x80 << (8 * (WB - 1 - fill % WB)) : (W)0;
  // the length field needs LEN_BYTES behind the 0x80: otherwise it goes into a block of its own
#pragma unroll 1
  for (int pass = (fill + 1 + H::LEN_BYTES > BB) ? 0 : 1; pass < 2; pass++) {
    if (pass == 1) {
      if constexpr (sizeof(W) == 4) {
        s.w[14] = s.total >> 29;
        s.w[15] = s.total << 3;
      } else {
        s.w[15] = (W)s.total << 3;
      }
    }
    compress<H>(s.h, s.w);
    clear_block(s);
  }
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = s.h[i];
}

// byte i of the big-endian form of the state words
template <class H>
ECGPU_HD u32 digest_byte(const typename H::W* d, u32 i) {
  constexpr u32 WB = sizeof(typename H::W);
  typename H::W w = d[0];
#pragma unroll
  for (u32 j = 1; j < 8; j++) w = (i / WB == j) ? d[j] : w;
  return (u32)(w >> (8 * (WB - 1 - i % WB))) & 0xFFu;
}

// Word-wise placement for messages whose layout is known when the code is written (hmac_drbg.hpp: HMAC and the RFC 6979 DRBG).
// m is a message as big-endian words, zeros where nothing has been placed yet, whole blocks long.  `pos` and `len` are byte
// positions in it and are literals at every device call, so that after inlining and unrolling every index into m is a constant: a
// secret word goes to one or two fixed slots by a fixed shift, and no load is addressed by a position as in `update`.
template <class H>
ECGPU_HD void place_word(typename H::W* m, u32 pos, typename H::W word) {
  constexpr u32 WB = sizeof(typename H::W);
  const u32 j = pos / WB, sh = 8 * (pos % WB);
  m[j] |= word >> sh;
  if (sh) m[j + 1] |= word << (8 * WB - sh);
}
template <class H>
ECGPU_HD void place_byte(typename H::W* m, u32 pos, u32 byte) {
  constexpr u32 WB = sizeof(typename H::W);
  m[pos / WB] |= (typename H::W)byte << (8 * (WB - 1 - pos % WB));
}
// blocks that a message of len bytes fills once padded
template <class H>
ECGPU_HD constexpr u32 padded_blocks(u32 len) { return (len + 1 + H::LEN_BYTES + H::BLOCK_BYTES - 1) / H::BLOCK_BYTES; }
// the 0x80 and the bit length of a message of len bytes that follows `prefix_blocks` blocks already compressed (lengths far below 2^29)
template <class H>
ECGPU_HD void pad_message(typename H::W* m, u32 len, u32 prefix_blocks) {
  place_byte<H>(m, len, 0x80u);
  m[16 * padded_blocks<H>(len) - 1] |= (typename H::W)((prefix_blocks * H::BLOCK_BYTES + len) << 3);
}

// one-shot
template <class H>
ECGPU_HD void hash(typename H::W* out, const uint8_t* p, u32 len) {
  State<H> s;
  init(s);
  update(s, p, len);
  finish(s, out);
}

}  // namespace sha2
}  // namespace ecgpu
