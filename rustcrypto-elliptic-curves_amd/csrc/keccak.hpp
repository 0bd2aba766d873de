// The Keccak-f[1600] sponge (FIPS 202; the Keccak team's original padding for Keccak-256) for one message per lane: the digests
// that the message-level ECDSA calls take besides the curve's own SHA-2 (ecgpu_ecdsa_*_digest_batch, ecgpu_digest_batch).  One
// template over (rate, domain byte, digest bytes):
//
//   Keccak256   rate 136   domain 0x01   32 bytes    the `sha3` crate's Keccak256, Ethereum's hash (k256/src/ecdsa.rs:84-143)
//   Sha3_256    rate 136   domain 0x06   32 bytes    FIPS 202
//   Sha3_384    rate 104   domain 0x06   48 bytes    FIPS 202
//
// Keccak-256 and SHA3-256 differ in the domain byte and in nothing else.
//
// Register shape: the state is 25 64-bit lanes, a[x + 5 y].  Every index into it is a compile-time constant: the rho offsets and
// the pi permutation are constexpr tables that the unrolled loops over the 25 lanes resolve, and a message byte is placed by
// comparing its position with every slot of the rate, not by indexing (a runtime-indexed private array would live in scratch).
// The 24 rounds run in a loop that is NOT unrolled; the round constant is read from a table by the (wave-uniform) round counter.
// One round is 260 vector instructions; unrolled, a kernel - the permutation is inlined three times: byte path, word path, padding -
// is 62 KiB of code against 13 KiB, at the same registers, and measures no faster at any shape: a round gains nothing from knowing
// its number (profiles/keccak_digest.txt).
//
// A lane is rotated by a constant on its two register halves (sha2.hpp rotr(u64)): two v_alignbit_b32, no 64-bit shift; no rho
// offset is 32, and the offset 0 of lane 0 is no rotation at all.
//
// Lanes are little-endian, so message words enter without a byte swap and the digest leaves without one.
//
// Constant time in the message: no branch and no address depends on a message byte.  Lengths are public: they steer the loops, the
// padding and the addresses of the byte loads.  So is the address of a message: update_aligned reads the whole blocks of a 4-byte
// aligned message by words.  Everything is ECGPU_HD: tests/hosttwin/hosttwin_keccak.cpp compiles the same text for the host.
#pragma once
#include "sha2.hpp"

namespace ecgpu {
namespace keccak {

template <int RATE, u32 DOMAIN, int DIGEST>
struct Sponge {
  static constexpr int RATE_BYTES = RATE, DIGEST_BYTES = DIGEST, LANES = RATE / 8;
  static constexpr u32 DOMAIN_BYTE = DOMAIN;
  static_assert(RATE % 8 == 0 && RATE < 200 && DIGEST % 8 == 0 && DIGEST <= RATE && RATE + 2 * DIGEST == 200, "capacity = twice the digest; whole lanes");
};
using Keccak256 = Sponge<136, 0x01u, 32>;
using Sha3_256 = Sponge<136, 0x06u, 32>;
using Sha3_384 = Sponge<104, 0x06u, 48>;

struct F1600 {
  // rho: lane x + 5 y is rotated left by RHO[x + 5 y]
  static constexpr int RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
  // pi: lane x + 5 y goes to lane PI[x + 5 y] = y + 5 ((2 x + 3 y) mod 5)
  static constexpr int PI[25] = {0, 10, 20, 5, 15, 16, 1, 11, 21, 6, 7, 17, 2, 12, 22, 23, 8, 18, 3, 13, 14, 24, 9, 19, 4};
  // iota
  static constexpr u64 RC[24] = {
      0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull, 0x0000000080000001ull,
      0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
      0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
      0x000000000000800Aull, 0x800000008000000Aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  // the tables against their definitions: rho walks (x, y) -> (y, 2 x + 3 y) from (1, 0) with the triangular numbers
  static constexpr bool tables_hold() {
    bool ok = RHO[0] == 0;
    int x = 1, y = 0;
    for (int t = 0; t < 24; t++) {
      ok = ok && RHO[x + 5 * y] == ((t + 1) * (t + 2) / 2) % 64 && RHO[x + 5 * y] % 32 != 0;
      const int ny = (2 * x + 3 * y) % 5;
      x = y;
      y = ny;
    }
    for (int i = 0; i < 25; i++) ok = ok && PI[i] == i / 5 + 5 * ((2 * (i % 5) + 3 * (i / 5)) % 5);
    return ok;
  }
};
static_assert(F1600::tables_hold(), "rho offsets and pi permutation");

// n is a literal after unrolling; never a multiple of 32 but 0
ECGPU_HD u64 rotl(u64 x, int n) { return n == 0 ? x : sha2::rotr(x, 64 - n); }

ECGPU_HD void round(u64* a, u64 rc) {
  u64 c[5], b[25];
#pragma unroll
  for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
  for (int x = 0; x < 5; x++) {
    const u64 d = c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1);
#pragma unroll
    for (int y = 0; y < 25; y += 5) a[x + y] ^= d;
  }
#pragma unroll
  for (int i = 0; i < 25; i++) b[F1600::PI[i]] = rotl(a[i], F1600::RHO[i]);
#pragma unroll
  for (int y = 0; y < 25; y += 5) {
#pragma unroll
    for (int x = 0; x < 5; x++) a[x + y] = b[x + y] ^ (~b[(x + 1) % 5 + y] & b[(x + 2) % 5 + y]);
  }
  a[0] ^= rc;
}
ECGPU_HD void permute(u64* a) {
#pragma unroll 1
  for (int r = 0; r < 24; r++) round(a, F1600::RC[r]);
}

// Incremental hashing: the bytes of the unfinished block are already XORed into the state; fill counts them (public).
template <class H>
struct State {
  u64 a[25];
  u32 fill;
};
template <class H>
ECGPU_HD void init(State<H>& s) {
#pragma unroll
  for (int i = 0; i < 25; i++) s.a[i] = 0;
  s.fill = 0;
}

// takes len bytes at p (any alignment).  One pass per block: every byte position of the rate that lies in [fill, fill + take) gets
// its byte; positions outside read p[off] (a byte that exists) and discard it, so the loads need no branch and stay in bounds.
template <class H>
ECGPU_HD void update(State<H>& s, const uint8_t* p, u32 len) {
  constexpr u32 RB = H::RATE_BYTES;
  u32 fill = s.fill, off = 0;
#pragma unroll 1
  while (off < len) {
    const u32 room = RB - fill, left = len - off;
    const u32 take = left < room ? left : room;
#pragma unroll
    for (u32 j = 0; j < (u32)H::LANES; j++) {
      u32 half[2] = {0u, 0u};
#pragma unroll
      for (u32 k = 0; k < 8; k++) {
        const u32 rel = j * 8 + k - fill;                // wraps for positions before `fill`: then rel >= take
        const bool in = rel < take;
        const u32 v = p[off + (in ? rel : 0u)];
        half[k / 4] |= (in ? v : 0u) << (8 * (k % 4));
      }
      s.a[j] ^= (u64)half[1] << 32 | half[0];
    }
    off += take;
    fill += take;
    if (fill == RB) {
      permute(s.a);
      fill = 0;
    }
  }
  s.fill = fill;
}
// one naturally aligned 32-bit load: lanes are little-endian, and so are the machines this is compiled for
ECGPU_HD u32 load_le32(const uint8_t* p) {
  u32 v;
  __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
  return v;
}
// `update` for whole messages: where the state stands at a block boundary and p is 4-byte aligned, every whole block comes in by
// RATE / 4 aligned 32-bit loads (34, SHA3-384: 26) instead of one load and RATE compares per byte; the partial last block, and
// everything where either condition fails, goes through `update` as it stands.  Which way a message goes depends on its address
// and on lengths alone (public); the word loads lie inside [p, p + len) and round no address (the rate is a multiple of 4).
template <class H>
ECGPU_HD void update_aligned(State<H>& s, const uint8_t* p, u32 len) {
  constexpr u32 RB = H::RATE_BYTES;
  static_assert(RB % 4 == 0, "a block after an aligned block is aligned");
  const bool words = s.fill == 0 && ((uintptr_t)p & 3u) == 0;
  const u32 whole = words ? len / RB : 0u;
#pragma unroll 1
  for (u32 b = 0; b < whole; b++) {
    const uint8_t* q = p + b * RB;
#pragma unroll
    for (u32 j = 0; j < (u32)H::LANES; j++) s.a[j] ^= (u64)load_le32(q + 8 * j + 4) << 32 | load_le32(q + 8 * j);
    permute(s.a);
  }
  update(s, p + whole * RB, len - whole * RB);
}
// pad10*1 behind the domain bits: the domain byte at the fill, 0x80 on the last byte of the rate (one byte, 0x81 / 0x86, where the
// two meet), and the last permutation.  The digest is then the first DIGEST_BYTES of the state, lanes in order, little-endian.
template <class H>
ECGPU_HD void finish(State<H>& s) {
  const u32 word = s.fill >> 2, d = H::DOMAIN_BYTE << (8 * (s.fill & 3u));
#pragma unroll
  for (u32 j = 0; j < (u32)H::LANES; j++) s.a[j] ^= (u64)(word == 2 * j + 1 ? d : 0u) << 32 | (word == 2 * j ? d : 0u);
  s.a[H::LANES - 1] ^= 0x8000000000000000ull;
  permute(s.a);
  s.fill = 0;
}

// The digest of one message as DIGEST_BYTES / 4 words as they lie in memory (out is 4-byte aligned): the row h2c::digest_words leaves
// for SHA-2, which a prehash kernel reads as const uint32_t*.
template <class H>
ECGPU_HD void digest_words(u32* out, const uint8_t* msg, u32 msg_len) {
  State<H> s;
  init(s);
  update_aligned(s, msg, msg_len);
  finish(s);
#pragma unroll
  for (int j = 0; j < H::DIGEST_BYTES / 8; j++) {
    out[2 * j] = (u32)s.a[j];
    out[2 * j + 1] = (u32)(s.a[j] >> 32);
  }
}

}  // namespace keccak
}  // namespace ecgpu
