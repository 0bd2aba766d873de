// Batched scalar-field arithmetic (integers modulo the group order n) behind ecgpu_scalar_op_batch and
// ecgpu_scalar_reduce_batch: Scalar::{mul, square, add, sub, negate, invert, sqrt} (k256/src/arithmetic/scalar.rs:99-327,
// p256/src/arithmetic/scalar.rs:99-277, p384/src/arithmetic/scalar.rs), Reduce / ReduceNonZero (k256 scalar.rs:700-750,
// scalar/wide64.rs:120-222) and the reduction of FromOkm (hash2curve.rs).
//
// Everything runs on the Montgomery multiplication of scalar_mont.hpp.  Operands are usually secrets (keys, nonces), so no
// branch and no address depends on an operand: a non-canonical operand, a zero to invert and a non-residue are masks
// (mp_select), the exponents are public, and the only conditional branches of the kernels are loop bounds and `index < n`
// on the public batch size (profiles/scalar_ops_ct_branches.txt).
//
// The per-element functions are __host__ __device__ so that the host twin (tests/hosttwin) compiles the same code.
#pragma once
#include "scalar_mont.hpp"

// Elements per lane that share one inversion in scalar_inv_kernel (Montgomery's trick: ~3 multiplications per element plus
// one Fermat inversion of ~320 per lane).  A/B: make variant NAME=... TU=ops_k256 DEFS=-DSCALAR_INV_BATCH=16.
// MI355X, 10^6 inversions / s at batch 1 / 8 / 16 / 32 (profiles/scalar_ops.txt): 2^24 elements k256 375 / 2369 / 3907 / 5541,
// p384 119 / 862 / 1512 / 2354; 2^20 elements k256 325 / 1879 / 2326 / 1866 (at 32 a 2^20 batch fills half the CUs).
#ifndef SCALAR_INV_BATCH
#define SCALAR_INV_BATCH 32
#endif

namespace ecgpu {

enum { SC_MUL = 0, SC_SQR = 1, SC_ADD = 2, SC_SUB = 3, SC_NEG = 4, SC_INV = 5, SC_SQRT = 6 };   // ecgpu_scalar_op
enum { SC_REDUCE_NONZERO = 1 };                                                                  // ECGPU_REDUCE_NONZERO

// Per-order constants of the square root and of the nonzero reduction:
//   S, ROOT  n - 1 = 2^S t; ROOT = MULTIPLICATIVE_GENERATOR^t (ROOT_OF_UNITY) in Montgomery form (k256 scalar.rs:349-353,
//            p256 scalar.rs:291-295)
//   EXP      exponent of the first power: (t - 1) / 2 for Tonelli-Shanks (k256 scalar.rs:292-297, p256 scalar.rs:242-247),
//            (n + 1) / 4 for P-384 (p384 scalar.rs:129-...; n = 3 mod 4)
//   C, CW    2^(32 L) mod (n - 1), CW words; NF folds X = H 2^(32 L) + Lo -> H C + Lo take any X < 2^(64 L) below 2^(32 L)
//            (the bound of each fold: tests/test_hosttwin_scalar_ops.py)
template <class O> struct ScalarAux;
template <> struct ScalarAux<K256Order> {
  static constexpr int S = 6;
  static constexpr u32 ROOT[8] = {0x20910E04u, 0x944CF2A2u, 0x780589F4u, 0x815C829Cu, 0xBC222113u, 0x55980B07u, 0x48825B36u, 0xC702B0D2u};
  static constexpr u32 EXP[8] = {0x19A06C82u, 0x777FA4BDu, 0xCD5E9140u, 0xFD755DB9u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x01FFFFFFu};
  static constexpr int CW = 5, NF = 4;
  static constexpr u32 C[5] = {0x2FC9BEC0u, 0x402DA173u, 0x50B75FC4u, 0x45512319u, 0x00000001u};
};
template <> struct ScalarAux<P256Order> {
  static constexpr int S = 4;
  static constexpr u32 ROOT[8] = {0x7E368FE1u, 0x1015708Fu, 0x6ECC4511u, 0x31C6C545u, 0x98A19EA1u, 0x5281FE89u, 0x10C63FE8u, 0x0279089Eu};
  static constexpr u32 EXP[8] = {0x17E3192Au, 0x279DCE56u, 0x6D38BCF4u, 0xFDE737D5u, 0xFFFFFFFFu, 0x07FFFFFFu, 0xF8000000u, 0x07FFFFFFu};
  static constexpr int CW = 7, NF = 9;
  static constexpr u32 C[7] = {0x039CDAB0u, 0x0C46353Du, 0x58E8617Bu, 0x43190552u, 0x00000000u, 0x00000000u, 0xFFFFFFFFu};
};
template <> struct ScalarAux<P384Order> {
  static constexpr int S = 1;
  static constexpr u32 ROOT[12] = {0x998A52E6u, 0xD9D832D5u, 0x91614EF5u, 0xB0341B64u, 0xE86E5BBEu, 0x8EC69B03u,
                                   0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  static constexpr u32 EXP[12] = {0xB3314A5Du, 0xBB3B065Au, 0x922C29DEu, 0xD606836Cu, 0x7D0DCB77u, 0xF1D8D360u,
                                  0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x3FFFFFFFu};
  static constexpr int CW = 6, NF = 3;
  static constexpr u32 C[6] = {0x333AD68Eu, 0x1313E695u, 0xB74F5885u, 0xA7E5F24Du, 0x0BC8D220u, 0x389CB27Eu};
};

namespace smont {

// r = a - b mod n; a, b < n
template <class O>
ECGPU_HD void sub(u32* r, const u32* a, const u32* b) {
  constexpr int L = O::L;
  u32 n[L], t[L], s[L];
  order<O>(n);
  const u32 bw = mp_sub<L>(t, a, b);
  (void)mp_add<L>(s, t, n);
  mp_select<L>(r, bw != 0, s, t);
}
// r = -a mod n; a < n
template <class O>
ECGPU_HD void neg(u32* r, const u32* a) {
  constexpr int L = O::L;
  u32 n[L], t[L], z[L];
  order<O>(n);
  (void)mp_sub<L>(t, n, a);
  mp_zero<L>(z);
  mp_select<L>(r, mp_is_zero<L>(a), z, t);
}
// r = a^e in Montgomery form for a PUBLIC exponent e (L words), 4-bit fixed windows.  Entry 0 of the table is ONE, so every
// window multiplies: no branch on the exponent either.
template <class O>
ECGPU_HD void pow_public(u32* r, const u32* a, const u32* e) {
  constexpr int L = O::L;
  u32 tab[16][L];
#pragma unroll
  for (int i = 0; i < L; i++) tab[0][i] = O::ONE[i];
  mp_copy<L>(tab[1], a);
#pragma unroll 1
  for (int i = 2; i < 16; i++) mul<O>(tab[i], tab[i - 1], a);
  u32 acc[L];
  mp_copy<L>(acc, tab[0]);
#pragma unroll 1
  for (int j = 8 * L - 1; j >= 0; j--) {
#pragma unroll 1
    for (int s = 0; s < 4; s++) mul<O>(acc, acc, acc);
    u32 w = e[0];
#pragma unroll
    for (int q = 1; q < L; q++) w = (j >> 3) == q ? e[q] : w;
    mul<O>(acc, acc, tab[(w >> (4 * (j & 7))) & 15u]);
  }
  mp_copy<L>(r, acc);
}

}  // namespace smont

namespace scops {

// x < n: keeps x and returns 1; otherwise clears x and returns 0 (from_repr rejects it)
template <class O>
ECGPU_HD u32 canon(u32* x) {
  constexpr int L = O::L;
  u32 n[L], z[L];
  smont::order<O>(n);
  mp_zero<L>(z);
  const bool ok = !mp_geq<L>(x, n);
  mp_select<L>(x, ok, x, z);
  return ok ? 1u : 0u;
}
// plain x plain -> plain: (a b R^-1) R^2 R^-1
template <class O>
ECGPU_HD void mul_plain(u32* r, const u32* a, const u32* b) {
  constexpr int L = O::L;
  u32 t[L], r2[L];
#pragma unroll
  for (int i = 0; i < L; i++) r2[i] = O::R2[i];
  smont::mul<O>(t, a, b);
  smont::mul<O>(r, t, r2);
}

// Field::sqrt on a Montgomery-form a; writes the reference's root (Montgomery form) and returns x^2 == a.  S > 1: the
// reference's constant-time Tonelli-Shanks (k256 scalar.rs:290-327, p256 scalar.rs:240-277), statement for statement with
// its conditional_select as masks; S = 1 (P-384): a^((n+1)/4).
template <class O>
ECGPU_HD bool sqrt_mont(u32* x, const u32* a) {
  using A = ScalarAux<O>;
  constexpr int L = O::L;
  u32 e[L], w[L], one[L];
#pragma unroll
  for (int i = 0; i < L; i++) { e[i] = A::EXP[i]; one[i] = O::ONE[i]; }
  smont::pow_public<O>(w, a, e);
  if constexpr (A::S == 1) {
    mp_copy<L>(x, w);
  } else {
    u32 b[L], z[L];
    smont::mul<O>(x, a, w);
    smont::mul<O>(b, x, w);
#pragma unroll
    for (int i = 0; i < L; i++) z[i] = A::ROOT[i];
    u32 v = A::S;
#pragma unroll 1
    for (int max_v = A::S; max_v >= 1; max_v--) {
      u32 k = 1, tmp[L];
      bool jlt = true;
      smont::mul<O>(tmp, b, b);
#pragma unroll 1
      for (int j = 2; j < max_v; j++) {
        const bool tio = mp_eq<L>(tmp, one);
        u32 sel[L], sq[L], nz[L];
        mp_select<L>(sel, tio, z, tmp);
        smont::mul<O>(sq, sel, sel);
        mp_select<L>(tmp, tio, tmp, sq);
        mp_select<L>(nz, tio, sq, z);
        jlt = jlt & ((u32)j != v);
        k = tio ? k : (u32)j;
        mp_select<L>(z, jlt, nz, z);
      }
      u32 res[L];
      smont::mul<O>(res, x, z);
      mp_select<L>(x, mp_eq<L>(b, one), x, res);
      smont::mul<O>(z, z, z);
      smont::mul<O>(b, b, z);
      v = k;
    }
  }
  u32 x2[L];
  smont::mul<O>(x2, x, x);
  return mp_eq<L>(x2, a);
}

// One element of an element-wise op (every op but SC_INV, which shares its inversion: inv_lane).  a, b, r: plain little-endian
// limbs; b is read for the binary ops only.  Returns ok (1 / 0); r is 0 where ok is 0.
template <class O, int OP>
ECGPU_HD u32 elem(u32* r, const u32* a_in, const u32* b_in) {
  static_assert(OP != SC_INV, "inversions go through inv_lane");
  constexpr int L = O::L;
  constexpr bool BIN = OP == SC_MUL || OP == SC_ADD || OP == SC_SUB;
  u32 a[L], b[L];
  mp_copy<L>(a, a_in);
  u32 ok = canon<O>(a);
  if constexpr (BIN) {
    mp_copy<L>(b, b_in);
    ok &= canon<O>(b);
  }
  if constexpr (OP == SC_MUL) mul_plain<O>(r, a, b);
  if constexpr (OP == SC_SQR) mul_plain<O>(r, a, a);
  if constexpr (OP == SC_ADD) smont::add<O>(r, a, b);
  if constexpr (OP == SC_SUB) smont::sub<O>(r, a, b);
  if constexpr (OP == SC_NEG) smont::neg<O>(r, a);
  if constexpr (OP == SC_SQRT) {
    u32 m[L], x[L];
    smont::to_mont<O>(m, a);
    ok &= sqrt_mont<O>(x, m) ? 1u : 0u;
    smont::from_mont<O>(r, x);
  }
  u32 z[L];
  mp_zero<L>(z);
  mp_select<L>(r, ok != 0, r, z);
  return ok;
}

// Masked batched inversion of cnt <= BATCH plain scalars, in place (Montgomery's trick, one smont::inv).  A zero or
// non-canonical element enters the prefix products as ONE, so it cannot poison the others, and leaves as 0.  Returns the
// mask of the elements that had an inverse (bit b = element b).
template <class O, int BATCH>
ECGPU_HD u32 inv_lane(u32 (*v)[O::L], int cnt) {
  static_assert(BATCH >= 1 && BATCH <= 32, "one mask bit per element");
  constexpr int L = O::L;
  u32 pre[BATCH][L], acc[L], one[L];
#pragma unroll
  for (int i = 0; i < L; i++) one[i] = O::ONE[i];
  mp_copy<L>(acc, one);
  u32 good = 0;
#pragma unroll 1
  for (int b = 0; b < cnt; b++) {
    u32 x[L];
    mp_copy<L>(x, v[b]);
    const u32 ok = canon<O>(x) & (mp_is_zero<L>(x) ? 0u : 1u);
    smont::to_mont<O>(v[b], x);
    mp_select<L>(v[b], ok != 0, v[b], one);
    good |= ok << b;
    mp_copy<L>(pre[b], acc);
    smont::mul<O>(acc, acc, v[b]);
  }
  u32 ai[L];
  smont::inv<O>(ai, acc);
#pragma unroll 1
  for (int b = cnt - 1; b >= 0; b--) {
    u32 t[L], z[L];
    smont::mul<O>(t, ai, pre[b]);
    smont::mul<O>(ai, ai, v[b]);
    smont::from_mont<O>(v[b], t);
    mp_zero<L>(z);
    mp_select<L>(v[b], ((good >> b) & 1u) != 0, v[b], z);
  }
  return good;
}

// A big-endian record of in_bytes (1 .. 8 L, a public length) bytes -> 2 L little-endian words, zero-extended
template <class O>
ECGPU_HD void load_wide(u32* w, const uint8_t* p, int in_bytes) {
  constexpr int L = O::L;
#pragma unroll
  for (int i = 0; i < 2 * L; i++) w[i] = 0;
#pragma unroll
  for (int j = 0; j < 8 * L; j++)
    if (j < in_bytes) w[j >> 2] |= (u32)p[in_bytes - 1 - j] << (8 * (j & 3));
}
// Reduce<U256 | U384 | U512>, FromOkm: r = w mod n for w < 2^(64 L).  Both halves are below 2n (n > 2^(32 L - 1) for
// the three orders), and H 2^(32 L) = mul(H, R^2) mod n.
template <class O>
ECGPU_HD void reduce_wide(u32* r, const u32* w) {
  constexpr int L = O::L;
  u32 h[L], lo[L], r2[L];
  mp_copy<L>(lo, w);
  mp_copy<L>(h, w + L);
#pragma unroll
  for (int i = 0; i < L; i++) r2[i] = O::R2[i];
  smont::reduce_once<O>(h);
  smont::reduce_once<O>(lo);
  smont::mul<O>(h, h, r2);
  smont::add<O>(r, h, lo);
}
// ReduceNonZero (wide64.rs:219-221): r = w mod (n - 1) + 1.  n - 1 is even, so no Montgomery reduction: NF folds by
// C = 2^(32 L) mod (n - 1) bring w below 2^(32 L) < 2 (n - 1), one conditional subtraction finishes.
template <class O>
ECGPU_HD void reduce_nonzero(u32* r, const u32* w) {
  using A = ScalarAux<O>;
  constexpr int L = O::L, CW = A::CW;
  u32 x[2 * L];
  mp_copy<2 * L>(x, w);
#pragma unroll
  for (int f = 0; f < A::NF; f++) {
    u32 p[2 * L], y[2 * L];
#pragma unroll
    for (int i = 0; i < 2 * L; i++) { p[i] = 0; y[i] = i < L ? x[i] : 0u; }
#pragma unroll
    for (int i = 0; i < L; i++) {            // p = H C, schoolbook by rows
      u64 carry = 0;
#pragma unroll
      for (int j = 0; j < CW; j++) {
        const u64 t = (u64)x[L + i] * A::C[j] + p[i + j] + carry;
        p[i + j] = (u32)t;
        carry = t >> 32;
      }
      if (i + CW < 2 * L) p[i + CW] = (u32)carry;
    }
    (void)mp_add<2 * L>(x, y, p);
  }
  u32 n1[L], d[L], one[L];
  smont::order<O>(n1);
  n1[0] -= 1;                                   // every order here is odd
  const u32 bw = mp_sub<L>(d, x, n1);
  mp_select<L>(d, bw == 0, d, x);
  mp_zero<L>(one);
  one[0] = 1;
  (void)mp_add<L>(r, d, one);
}

}  // namespace scops

#if defined(__HIPCC__)
// big-endian word strings of L words, as the other kernels take them (traits.hpp words_load_be)
template <int L>
__device__ __forceinline__ void sc_load_be(u32* limbs, const u32* be) {
#pragma unroll
  for (int i = 0; i < L; i++) limbs[i] = bswap32(be[L - 1 - i]);
}
template <int L>
__device__ __forceinline__ void sc_store_be(u32* be, const u32* limbs) {
#pragma unroll
  for (int i = 0; i < L; i++) be[L - 1 - i] = bswap32(limbs[i]);
}

// element-wise ops: one lane per element on a grid stride; ok may be NULL
template <class O, int OP>
__global__ void __launch_bounds__(256) scalar_op_kernel(const u32* a, const u32* b, u32* out, uint8_t* ok, size_t n) {
  constexpr int L = O::L;
  constexpr bool BIN = OP == SC_MUL || OP == SC_ADD || OP == SC_SUB;
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) {
    u32 x[L], y[L], r[L];
    sc_load_be<L>(x, a + i * L);
    if constexpr (BIN) sc_load_be<L>(y, b + i * L);
    else mp_zero<L>(y);
    const u32 g = scops::elem<O, OP>(r, x, y);
    sc_store_be<L>(out + i * L, r);
    if (ok) ok[i] = (uint8_t)g;
  }
}
// inversion: each lane takes BATCH elements one grid stride apart (like verify_prep_kernel) and inverts them with one
// Fermat inversion; the last batch of a lane may be partial (cnt < BATCH)
template <class O, int BATCH>
__global__ void __launch_bounds__(256) scalar_inv_kernel(const u32* a, u32* out, uint8_t* ok, size_t n) {
  constexpr int L = O::L;
  const size_t T = (size_t)gridDim.x * blockDim.x;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t base = tid; base < n; base += T * BATCH) {
    u32 v[BATCH][L];
    int cnt = 0;
#pragma unroll 1
    for (int b = 0; b < BATCH; b++) {
      const size_t i = base + (size_t)b * T;
      if (i >= n) break;
      sc_load_be<L>(v[b], a + i * L);
      cnt = b + 1;
    }
    const u32 good = scops::inv_lane<O, BATCH>(v, cnt);
#pragma unroll 1
    for (int b = 0; b < cnt; b++) {
      const size_t i = base + (size_t)b * T;
      sc_store_be<L>(out + i * L, v[b]);
      if (ok) ok[i] = (uint8_t)((good >> b) & 1u);
    }
  }
}
// Reduce / ReduceNonZero of n big-endian records of in_bytes bytes (any alignment)
template <class O, bool NONZERO>
__global__ void __launch_bounds__(256) scalar_reduce_kernel(const uint8_t* in, int in_bytes, u32* out, size_t n) {
  constexpr int L = O::L;
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) {
    u32 w[2 * L], r[L];
    scops::load_wide<O>(w, in + i * (size_t)in_bytes, in_bytes);
    if constexpr (NONZERO) scops::reduce_nonzero<O>(r, w);
    else scops::reduce_wide<O>(r, w);
    sc_store_be<L>(out + i * L, r);
  }
}
#endif

}  // namespace ecgpu
