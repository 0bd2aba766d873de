// TEST-ONLY host build of BIP340 batch verification's term preparation (schnorr_batch_kernels.hpp): the coefficient, the lane body
// of prep_kernel and the wide modular sum, run in the kernel's shape - lanes on a grid stride, 64 lanes to a wave, four waves to a
// workgroup, one partial per workgroup, then the finish step.  Checked against tests/schnorr_batch_model.py and the oracle by
// tests/test_hosttwin_schnorr_batch.py; with -DHOSTTWIN_SCHNORR_BATCH_MAIN the file is a program of its own (for a sanitizer build: schnorr_batch_san.mk).
#ifndef HOSTTWIN_SCHNORR_BATCH_MAIN
#include "hosttwin_trace.hpp"      // in the library every translation unit builds the shared inline functions with the same hooks
#endif
#include <string.h>
#include <vector>
#include "schnorr_batch_kernels.hpp"
using namespace ecgpu;
namespace sb = ecgpu::schnorr_batch;

namespace {
sb::Seed seed_from(const uint8_t* seed32) {
  sb::Seed s;
  for (int i = 0; i < 8; i++) s.w[i] = (u32)seed32[4 * i] << 24 | (u32)seed32[4 * i + 1] << 16 | (u32)seed32[4 * i + 2] << 8 | (u32)seed32[4 * i + 3];
  return s;
}
struct Acc {
  u32 w[sb::SUMW] = {};
  u32 bad = 0;
};
// the workgroups' partials of `lanes` lanes (a multiple of 256) folded as the kernels fold them: lanes into waves, waves into
// workgroups, workgroups into the one accumulator of the finish step
Acc fold(const std::vector<Acc>& lane) {
  Acc total;
  for (size_t b = 0; b < lane.size(); b += 256) {
    Acc wg;
    for (int wv = 0; wv < 4; wv++) {
      Acc wave;
      for (int l = 0; l < 64; l++) { sb::sum_add<sb::SUMW>(wave.w, lane[b + 64 * wv + l].w); wave.bad += lane[b + 64 * wv + l].bad; }
      sb::sum_add<sb::SUMW>(wg.w, wave.w);
      wg.bad += wave.bad;
    }
    sb::sum_add<sb::SUMW>(total.w, wg.w);
    total.bad += wg.bad;
  }
  return total;
}
}  // namespace

extern "C" {
// a = the 16 coefficient bytes, big-endian
int ht_sb_coefficient(const uint8_t* seed32, uint64_t index, uint8_t* a16) {
  u32 a[8], be[8];
  sb::coefficient(a, seed_from(seed32), index);
  if (a[4] | a[5] | a[6] | a[7]) return -1;
  words_store_be<8>(be, a);
  memcpy(a16, (const uint8_t*)be + 16, 16);
  return 0;
}
// The terms of n signatures (px: n x 32, sig: n x 64, e: n x 32 bytes) on `lanes` lanes (a multiple of 256): sc = (2n + 1) x 32 bytes,
// pts = (2n + 1) x 64 bytes, dec = n bytes.  Returns the number of left-out elements.
int ht_sb_terms(const uint8_t* px, const uint8_t* sig, const uint8_t* e, const uint8_t* seed32, uint64_t first_index, size_t n, int lanes, uint8_t* sc,
                uint8_t* pts, uint8_t* dec) {
  if (lanes <= 0 || lanes % 256) return -1;
  const sb::Seed seed = seed_from(seed32);
  std::vector<Acc> lane((size_t)lanes);
  for (size_t i = 0; i < n; i++) {
    u32 pw[8], sw[16], ew[8], s[16], p[32], t[8];
    memcpy(pw, px + 32 * i, 32); memcpy(sw, sig + 64 * i, 64); memcpy(ew, e + 32 * i, 32);
    const u32 g = sb::prep_lane(s, p, t, pw, sw, ew, seed, first_index + i);
    memcpy(sc + 64 * i, s, 64);
    memcpy(pts + 128 * i, p, 128);
    dec[i] = (uint8_t)g;
    Acc& a = lane[i % (size_t)lanes];
    a.bad += 1u - g;
    sb::sum_add<8>(a.w, t);
  }
  const Acc total = fold(lane);
  u32 k[8], ks[8], gp[16];
  sb::sum_finish(k, total.w);
  sb::generator_term(ks, gp, k);
  memcpy(sc + 64 * n, ks, 32);
  memcpy(pts + 128 * n, gp, 64);
  return (int)total.bad;
}
// k = n - (sum of the cnt scalars mod n), 0 for a sum that is 0 mod n: scalars cnt x 32 bytes big-endian, below 2^256
int ht_sb_sum(const uint8_t* scalars, size_t cnt, int lanes, uint8_t* k32) {
  if (lanes <= 0 || lanes % 256) return -1;
  std::vector<Acc> lane((size_t)lanes);
  for (size_t i = 0; i < cnt; i++) {
    u32 be[8], t[8];
    memcpy(be, scalars + 32 * i, 32);
    words_load_be<8>(t, be);
    sb::sum_add<8>(lane[i % (size_t)lanes].w, t);
  }
  const Acc total = fold(lane);
  u32 k[8], be[8];
  sb::sum_finish(k, total.w);
  words_store_be<8>(be, k);
  memcpy(k32, be, 32);
  return 0;
}
}

#ifdef HOSTTWIN_SCHNORR_BATCH_MAIN
#include <stdio.h>
#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)
static void unhex(uint8_t* out, const char* hex, int bytes) {
  for (int i = 0; i < bytes; i++) { unsigned v; sscanf(hex + 2 * i, "%2x", &v); out[i] = (uint8_t)v; }
}
int main() {
  // BIP340 verify vector 4 (valid) and four ways of breaking its decoding; vector 5's key is no x-coordinate
  uint8_t pk[32], sg[64], msg[32], off_curve[32], order[32], prime[32];
  unhex(pk, "d69c3509bb99e412e68b0fe8544e72837dfa30746d8be2aa65975f29d22dc7b9", 32);
  unhex(sg, "00000000000000000000003b78ce563f89a0ed9414f5aa28ad0d96d6795f9c6376afb1548af603b3eb45c9f8207dee1060cb71c04e80f593060b07d28308d7f4", 64);
  unhex(msg, "4df3c3f68fcc83b27e9d42c90431a72499f17875c81a599b566c9889b9696703", 32);
  unhex(off_curve, "eefdea4cdb677750a420fee807eacf21eb9898ae79b9768766e4faa04a2d4a34", 32);
  unhex(order, "fffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141", 32);
  unhex(prime, "fffffffffffffffffffffffffffffffffffffffffffffffffffffffefffffc2f", 32);
  constexpr size_t N = 7;
  std::vector<uint8_t> px(32 * N), sig(64 * N), e(32 * N), sc(32 * (2 * N + 1)), pts(64 * (2 * N + 1)), dec(N);
  for (size_t i = 0; i < N; i++) { memcpy(&px[32 * i], pk, 32); memcpy(&sig[64 * i], sg, 64); }
  memcpy(&px[32 * 1], off_curve, 32);                 // key without a curve point
  memcpy(&sig[64 * 2], off_curve, 32);                // r is no x-coordinate
  memset(&sig[64 * 3], 0, 32);                        // r = 0
  memcpy(&sig[64 * 4 + 32], order, 32);               // s = n
  memcpy(&px[32 * 5], prime, 32);                     // key x = p
  for (size_t i = 0; i < N; i++) {
    u32 r[8], p[8], m[8], ew[8];
    memcpy(r, &sig[64 * i], 32); memcpy(p, &px[32 * i], 32); memcpy(m, msg, 32);
    h2c::bip340_challenge(ew, r, p, m);
    memcpy(&e[32 * i], ew, 32);
  }
  uint8_t seed[32];
  for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(7 * i + 1);
  const int bad = ht_sb_terms(px.data(), sig.data(), e.data(), seed, ((uint64_t)1 << 32) + 5, N, 256, sc.data(), pts.data(), dec.data());
  CHECK(bad == 5);
  const uint8_t want[N] = {1, 0, 0, 0, 0, 0, 1};
  for (size_t i = 0; i < N; i++) CHECK(dec[i] == want[i]);
  // a kept element: term 2i is (a_i, (r, even y)), a left-out one carries two zero scalars
  uint8_t a16[16];
  CHECK(ht_sb_coefficient(seed, ((uint64_t)1 << 32) + 5, a16) == 0);
  CHECK(memcmp(&sc[16], a16, 16) == 0 && memcmp(&pts[0], sg, 32) == 0 && (pts[63] & 1) == 0);
  for (int b = 0; b < 64; b++) CHECK(sc[64 * 1 + b] == 0);
  // m scalars n - 1 sum to -m: the generator term's scalar is m
  for (int m : {1, 2, 255, 256, 257, 1000}) {
    std::vector<uint8_t> s(32 * (size_t)m), k(32);
    for (int i = 0; i < m; i++) { memcpy(&s[32 * (size_t)i], order, 32); s[32 * (size_t)i + 31] -= 1; }
    for (int lanes : {256, 512}) {
      CHECK(ht_sb_sum(s.data(), (size_t)m, lanes, k.data()) == 0);
      for (int b = 0; b < 30; b++) CHECK(k[b] == 0);
      CHECK(k[30] == (m >> 8) && k[31] == (m & 255));
    }
  }
  printf("schnorr batch twin ok: %zu signatures, %d left out\n", N, bad);
  return 0;
}
#endif
