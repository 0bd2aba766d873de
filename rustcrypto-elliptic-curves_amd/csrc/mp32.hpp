// Multi-precision primitives on saturated 32-bit limbs for gfx950.
//
// Design notes (measured with tools/ubench/valu_rates.hip on MI355X):
//  * the native integer multiplier is v_mad_u64_u32 (32x32+64 -> 64, carry-out in an SGPR pair);
//    a u64 x u64 product lowers to four of them, so the natural limb is 32 bits and a field
//    element of a 256-bit (384-bit) prime lives in 8 (12) VGPRs of one lane;
//  * v_mad_u64_u32 has a carry-out but no carry-in and 64-bit VGPR operands must be even aligned,
//    so products are accumulated column-wise into a 96-bit accumulator: one mad plus one
//    v_addc_co_u32 per 32x32 multiply-accumulate.  hipcc does not form that pair from C++
//    (it emits mad + 64-bit add + compare + select), hence the two-instruction asm statement.
//
// Everything here is __host__ __device__: the same templates are compiled by the host compiler
// into tests/hosttwin (a test-only library) so that the arithmetic can be checked against the
// oracle in a container without a GPU.  The shipped library (libecgpu.so) only ever launches
// the device instantiation.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ECGPU_HD __host__ __device__ __forceinline__
#else
#define ECGPU_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define ECGPU_ASM 1
#else
#define ECGPU_ASM 0
#endif

// Hook at every read of a precomputed-table entry; empty in the product.  The test-only host build (tests/hosttwin)
// defines it to record the entry index, which is how the tests show that the constant-time schedules touch the same
// entries in the same order whatever the scalar is, and that the throughput schedules do not.
#ifndef ECGPU_TABLE_TOUCH
#define ECGPU_TABLE_TOUCH(idx) ((void)0)
#endif
// Hook at every exceptional case of the incomplete point additions (accumulator or addend at infinity, the same point, opposite
// points; "...:z" again while the accumulator's Z has left 1): empty in the product, and `cond` is NOT evaluated there.  The
// test-only host build counts, per site name, how often `cond` holds, which is how the tests show that their related-point inputs
// (tests/related_point_vectors.py) really enter these branches.
#ifndef ECGPU_EXC_NOTE
#define ECGPU_EXC_NOTE(site, cond) ((void)0)
#endif
// Hook at every speculative product of the k256 field products (fe_k256.hpp), after its column (the missing carry already added) and
// before its carry-out flag is merged with the others: empty in the product, and `raised` is NOT evaluated there.  The test-only host build records, per site name
// and column, whether the flag was raised, which is how the tests show that their inputs reach every rare carry branch.
#ifndef ECGPU_SPEC_NOTE
#define ECGPU_SPEC_NOTE(site, column, raised) ((void)0)
#endif
// Hook at the tail of every k256 reduction (fe_k256.hpp: the overflow word T on the carry chains, the fold of T * C, the rare ripple
// behind it): empty in the product, and `cond` is NOT evaluated there.  The test-only host build counts, per site name, how often
// `cond` holds, which is how the tests show that their operands reach both chain carries, word 16, the ripple and the second fold.
#ifndef ECGPU_TAIL_NOTE
#define ECGPU_TAIL_NOTE(site, cond) ((void)0)
#endif

namespace ecgpu {

typedef uint32_t u32;
typedef uint64_t u64;

// ---------------------------------------------------------------------------------------------
// carry chains.  __builtin_addc / __builtin_subc lower to v_add_co_u32 / v_addc_co_u32 chains.
// ---------------------------------------------------------------------------------------------
ECGPU_HD u32 addc(u32 a, u32 b, u32& carry) {
#if defined(__clang__)
  u32 co;
  u32 r = __builtin_addc(a, b, carry, &co);
  carry = co;
  return r;
#else
  u64 t = (u64)a + b + carry;
  carry = (u32)(t >> 32);
  return (u32)t;
#endif
}
ECGPU_HD u32 subb(u32 a, u32 b, u32& borrow) {
#if defined(__clang__)
  u32 bo;
  u32 r = __builtin_subc(a, b, borrow, &bo);
  borrow = bo;
  return r;
#else
  u64 t = (u64)a - b - borrow;
  borrow = (u32)(t >> 63);
  return (u32)t;
#endif
}

// r = a + b, returns carry-out
template <int N>
ECGPU_HD u32 mp_add(u32* r, const u32* a, const u32* b) {
  u32 c = 0;
#pragma unroll
  for (int i = 0; i < N; i++) r[i] = addc(a[i], b[i], c);
  return c;
}
// r = a - b, returns borrow-out
template <int N>
ECGPU_HD u32 mp_sub(u32* r, const u32* a, const u32* b) {
  u32 c = 0;
#pragma unroll
  for (int i = 0; i < N; i++) r[i] = subb(a[i], b[i], c);
  return c;
}
// a >= b ?
template <int N>
ECGPU_HD bool mp_geq(const u32* a, const u32* b) {
  u32 c = 0;
#pragma unroll
  for (int i = 0; i < N; i++) (void)subb(a[i], b[i], c);
  return c == 0;
}
template <int N>
ECGPU_HD bool mp_is_zero(const u32* a) {
  u32 t = 0;
#pragma unroll
  for (int i = 0; i < N; i++) t |= a[i];
  return t == 0;
}
template <int N>
ECGPU_HD bool mp_eq(const u32* a, const u32* b) {
  u32 t = 0;
#pragma unroll
  for (int i = 0; i < N; i++) t |= a[i] ^ b[i];
  return t == 0;
}
template <int N>
ECGPU_HD void mp_copy(u32* r, const u32* a) {
#pragma unroll
  for (int i = 0; i < N; i++) r[i] = a[i];
}
template <int N>
ECGPU_HD void mp_zero(u32* r) {
#pragma unroll
  for (int i = 0; i < N; i++) r[i] = 0;
}
// r = cond ? a : b   (lane-wise select, v_cndmask_b32)
template <int N>
ECGPU_HD void mp_select(u32* r, bool cond, const u32* a, const u32* b) {
#pragma unroll
  for (int i = 0; i < N; i++) r[i] = cond ? a[i] : b[i];
}

// ---------------------------------------------------------------------------------------------
// 96-bit column accumulator
// ---------------------------------------------------------------------------------------------
struct Acc96 {
  u64 lo;
  u32 hi;
};

// c += a * b
ECGPU_HD void mac(Acc96& c, u32 a, u32 b) {
#if ECGPU_ASM
  asm("v_mad_u64_u32 %0, vcc, %2, %3, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc"
      : "+v"(c.lo), "+v"(c.hi)
      : "v"(a), "v"(b)
      : "vcc");
#else
  u64 p = (u64)a * b;
  c.lo += p;
  c.hi += (c.lo < p);
#endif
}
// c += a * b where the caller guarantees the low 64 bits cannot overflow
ECGPU_HD void mac_nc(Acc96& c, u32 a, u32 b) { c.lo += (u64)a * b; }
// c.lo += a * b WITHOUT the carry into c.hi; returns whether the low 64 bits wrapped (portable twin of the speculative product of the
// mac_colM_nN_s1 forms, whose device form returns the mad's carry-out lane mask).  mac_spec_fix adds what it returns.
ECGPU_HD u64 mac_spec(Acc96& c, u32 a, u32 b) {
  const u64 p = (u64)a * b;
  c.lo += p;
  return c.lo < p ? 1u : 0u;
}
// c.hi += the carry that a speculative product left in k (device: a lane mask, the carry-in of one v_addc_co_u32).  Additions
// commute, so it may come after the column's other products; it must come before the accumulator is popped.
ECGPU_HD void mac_spec_fix(Acc96& c, u64 k) {
#if ECGPU_ASM
  asm("v_addc_co_u32 %0, vcc, 0, %0, %1" : "+v"(c.hi) : "s"(k) : "vcc");
#else
  c.hi += (u32)k;
#endif
}
// c -= w, the accumulator read as a 96-bit two's-complement number
ECGPU_HD void acc_sub32(Acc96& c, u32 w) {
  u32 l0 = (u32)c.lo, l1 = (u32)(c.lo >> 32), bw = 0;
  l0 = subb(l0, w, bw);
  l1 = subb(l1, 0u, bw);
  c.hi = subb(c.hi, 0u, bw);
  c.lo = ((u64)l1 << 32) | l0;
}

#include "mp32_cols.inc"

// c += sum_{m < M} pa[m] * pb[m], issued as one asm statement.  FRESH: the caller knows c.hi == 0 (the accumulator was
// just popped or zeroed); the first carry then produces c.hi instead of adding to it, which saves zeroing a register
// per column.  NC: the caller knows that the first NC products cannot carry out of c.lo (each call site states the bound);
// they are issued without their carry addition.
template <int M, bool FRESH = false, int NC = 0>
ECGPU_HD void mac_cols(Acc96& c, const u32* pa, const u32* pb) {
  static_assert(M >= 1, "column length");
  static_assert(NC >= 0 && NC <= 2 && NC <= M, "at most two leading products without a carry");
  if constexpr (M > 12) {            // an asm statement takes at most 30 operands: split long columns
    mac_cols<12, FRESH, NC>(c, pa, pb);
    mac_cols<M - 12, false>(c, pa + 12, pb + 12);
  } else if constexpr (NC > 0) {
    mac_cols_nc<M, FRESH, NC>(c, pa, pb);
  } else {
    if constexpr (M == 1) { if constexpr (FRESH) mac_col1_f(c, pa[0], pb[0]); else mac_col1(c, pa[0], pb[0]); }
    if constexpr (M == 2) { if constexpr (FRESH) mac_col2_f(c, pa[0], pb[0], pa[1], pb[1]); else mac_col2(c, pa[0], pb[0], pa[1], pb[1]); }
    if constexpr (M == 3) { if constexpr (FRESH) mac_col3_f(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2]); else mac_col3(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2]); }
    if constexpr (M == 4) { if constexpr (FRESH) mac_col4_f(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3]); else mac_col4(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3]); }
    if constexpr (M == 5) { if constexpr (FRESH) mac_col5_f(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4]); else mac_col5(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4]); }
    if constexpr (M == 6) { if constexpr (FRESH) mac_col6_f(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4], pa[5], pb[5]); else mac_col6(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4], pa[5], pb[5]); }
    if constexpr (M == 7) { if constexpr (FRESH) mac_col7_f(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4], pa[5], pb[5], pa[6], pb[6]); else mac_col7(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4], pa[5], pb[5], pa[6], pb[6]); }
    if constexpr (M == 8) { if constexpr (FRESH) mac_col8_f(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4], pa[5], pb[5], pa[6], pb[6], pa[7], pb[7]); else mac_col8(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4], pa[5], pb[5], pa[6], pb[6], pa[7], pb[7]); }
    if constexpr (M == 9) { if constexpr (FRESH) mac_col9_f(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4], pa[5], pb[5], pa[6], pb[6], pa[7], pb[7], pa[8], pb[8]); else mac_col9(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4], pa[5], pb[5], pa[6], pb[6], pa[7], pb[7], pa[8], pb[8]); }
    if constexpr (M == 10) { if constexpr (FRESH) mac_col10_f(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4], pa[5], pb[5], pa[6], pb[6], pa[7], pb[7], pa[8], pb[8], pa[9], pb[9]); else mac_col10(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4], pa[5], pb[5], pa[6], pb[6], pa[7], pb[7], pa[8], pb[8], pa[9], pb[9]); }
    if constexpr (M == 11) { if constexpr (FRESH) mac_col11_f(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4], pa[5], pb[5], pa[6], pb[6], pa[7], pb[7], pa[8], pb[8], pa[9], pb[9], pa[10], pb[10]); else mac_col11(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4], pa[5], pb[5], pa[6], pb[6], pa[7], pb[7], pa[8], pb[8], pa[9], pb[9], pa[10], pb[10]); }
    if constexpr (M == 12) { if constexpr (FRESH) mac_col12_f(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4], pa[5], pb[5], pa[6], pb[6], pa[7], pb[7], pa[8], pb[8], pa[9], pb[9], pa[10], pb[10], pa[11], pb[11]); else mac_col12(c, pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[3], pb[3], pa[4], pb[4], pa[5], pb[5], pa[6], pb[6], pa[7], pb[7], pa[8], pb[8], pa[9], pb[9], pa[10], pb[10], pa[11], pb[11]); }
  }
}
// The same with SPEC: after the NC products comes one SPECULATIVE product (mac_colM_nN_s1).  It starts from an accumulator so small
// (the caller's bound) that its carry out of c.lo is rarer than 2^-40, so the column issues it WITHOUT its carry addition and keeps the
// mad's carry-out lane mask in a scalar-register pair; a wave-uniform branch, almost never taken, adds the missing carry when any
// lane's bit is set.  The value is exact either way; which way the branch goes depends on the data (not for secret inputs).  The mask
// (0 or 1 in the portable build) is OR-ed into `raised` for the caller's ECGPU_SPEC_NOTE.  Without SPEC this is mac_cols above.
template <int M, bool FRESH = false, int NC = 0, bool SPEC = false>
ECGPU_HD void mac_cols(Acc96& c, const u32* pa, const u32* pb, u64& raised) {
  if constexpr (!SPEC) {
    mac_cols<M, FRESH, NC>(c, pa, pb);
  } else {
    static_assert(M >= 1 && NC >= 0 && NC <= 2 && NC + 1 <= M, "the speculative product follows the no-carry products");
    u64 k;
    if constexpr (M > 12) {
      mac_cols_s1<12, FRESH, NC>(c, k, pa, pb);
      mac_cols<M - 12, false>(c, pa + 12, pb + 12);
    } else {
      mac_cols_s1<M, FRESH, NC>(c, k, pa, pb);
    }
    if (__builtin_expect(k != 0, 0)) mac_spec_fix(c, k);
    raised |= k;
  }
}
// column k of the N x N schoolbook product: sum_{i+j=k} a_i b_j, plus NX extra products (xa, xb) issued FIRST, so that a
// small extra product (the k256 fold term) can go in without a carry.  NC: the first NC products of that order (extras, then
// a_LO b_(k-LO), ..) cannot carry out of c.lo, as the caller states.
template <int N, int K, int NX, bool FRESH = false, int NC = 0>
ECGPU_HD void mac_product_column(Acc96& c, const u32* a, const u32* b, const u32* xa, const u32* xb) {
  constexpr int LO = (K - (N - 1)) > 0 ? (K - (N - 1)) : 0;
  constexpr int HI = K < (N - 1) ? K : (N - 1);
  constexpr int M = HI - LO + 1;
  u32 pa[M + NX + 1], pb[M + NX + 1];
#pragma unroll
  for (int m = 0; m < NX; m++) { pa[m] = xa[m]; pb[m] = xb[m]; }
#pragma unroll
  for (int m = 0; m < M; m++) { pa[NX + m] = a[LO + m]; pb[NX + m] = b[K - LO - m]; }
  mac_cols<M + NX, FRESH, NC>(c, pa, pb);
}
// SPEC: the product after the NC leading ones is speculative (mac_cols with `raised`)
template <int N, int K, int NX, bool FRESH = false, int NC = 0, bool SPEC = false>
ECGPU_HD void mac_product_column(Acc96& c, const u32* a, const u32* b, const u32* xa, const u32* xb, u64& raised) {
  constexpr int LO = (K - (N - 1)) > 0 ? (K - (N - 1)) : 0;
  constexpr int HI = K < (N - 1) ? K : (N - 1);
  constexpr int M = HI - LO + 1;
  u32 pa[M + NX + 1], pb[M + NX + 1];
#pragma unroll
  for (int m = 0; m < NX; m++) { pa[m] = xa[m]; pb[m] = xb[m]; }
#pragma unroll
  for (int m = 0; m < M; m++) { pa[NX + m] = a[LO + m]; pb[NX + m] = b[K - LO - m]; }
  mac_cols<M + NX, FRESH, NC, SPEC>(c, pa, pb, raised);
}

// pop the low word and shift the accumulator down by 32 bits
ECGPU_HD u32 acc_pop(Acc96& c) {
  u32 r = (u32)c.lo;
  c.lo = (c.lo >> 32) | ((u64)c.hi << 32);
  c.hi = 0;
  return r;
}

// the same for a signed accumulator (arithmetic shift)
ECGPU_HD u32 acc_pop_signed(Acc96& c) {
  u32 r = (u32)c.lo;
  c.lo = (c.lo >> 32) | ((u64)c.hi << 32);
  c.hi = (u32)((int32_t)c.hi >> 31);
  return r;
}

// r[0..2N) = a * b   (schoolbook, product scanning)
template <int N>
ECGPU_HD void mp_mul_wide(u32* r, const u32* a, const u32* b) {
  Acc96 c{0, 0};
#pragma unroll
  for (int k = 0; k < 2 * N - 1; k++) {
#pragma unroll
    for (int i = 0; i < N; i++) {
      const int j = k - i;
      if (j >= 0 && j < N) {
        if (k == 0 || k == 2 * N - 2) mac_nc(c, a[i], b[j]); else mac(c, a[i], b[j]);
      }
    }
    r[k] = acc_pop(c);
  }
  r[2 * N - 1] = (u32)c.lo;
}


// column K of the off-diagonal half of a square: sum_{i < j, i + j = K} a_i a_j
template <int N, int K>
ECGPU_HD void mac_cross_column(Acc96& c, const u32* a) {
  constexpr int LO = (K - (N - 1)) > 0 ? (K - (N - 1)) : 0;
  constexpr int HI = (K - 1) / 2;            // largest i with i < K - i
  constexpr int M = HI - LO + 1;
  if constexpr (M >= 1) {
    u32 pa[M], pb[M];
#pragma unroll
    for (int m = 0; m < M; m++) { pa[m] = a[LO + m]; pb[m] = a[K - LO - m]; }
    mac_cols<M, true>(c, pa, pb);        // every cross column starts from a popped (or zero) accumulator
  }
}
template <int N, int K>
ECGPU_HD void sqr_cross_columns(u32* x, Acc96& c, const u32* a) {
  if constexpr (K < 2 * N - 2) {
    mac_cross_column<N, K>(c, a);
    x[K] = acc_pop(c);
    sqr_cross_columns<N, K + 1>(x, c, a);
  }
}

// Whether the first product of cross column K of an N-word square cannot carry out of c.lo: the carry popped into the column for an
// all-ones operand (every column sum is monotone in the words) plus the largest product stays below 2^64.
template <int N>
constexpr bool sqr_cross_first_nc(int K) {
  typedef unsigned __int128 u128;
  const u128 maxp = (u128)0xFFFFFFFFu * 0xFFFFFFFFu;
  u128 c = 0;
  for (int k = 1; k < K; k++) {
    const int lo = (k - (N - 1)) > 0 ? (k - (N - 1)) : 0, hi = (k - 1) / 2;
    c = (c + (u128)(hi - lo + 1) * maxp) >> 32;
  }
  return c + maxp < ((u128)1 << 64);
}
// SPEC: the first product of a cross column is a no-carry product where sqr_cross_first_nc proves it (for N = 8: columns 1 to 5 and
// 11 to 13) and, in a column of two or more products, speculative elsewhere (mac_cols with `raised`).  A one-product column that is
// carry-free is written in C++ (mac_nc): the compiler's three-address mad takes the popped word from a pair with a standing zero,
// one move less than the asm column.  A one-product column that may carry (none for N = 8) stays exact: its carry addition is
// what creates c.hi, and without it a move would have to.
static_assert(sqr_cross_first_nc<8>(1) && sqr_cross_first_nc<8>(2) && sqr_cross_first_nc<8>(3) && sqr_cross_first_nc<8>(4) && sqr_cross_first_nc<8>(5) &&
              !sqr_cross_first_nc<8>(6) && !sqr_cross_first_nc<8>(10) && sqr_cross_first_nc<8>(11) && sqr_cross_first_nc<8>(12) && sqr_cross_first_nc<8>(13),
              "the carry-free cross columns of the 8-word square, as the comments and tests/k256_spec_carry_vectors.py list them");
template <int N, int K, bool SPEC>
ECGPU_HD void mac_cross_column(Acc96& c, const u32* a, u64& raised) {
  constexpr int LO = (K - (N - 1)) > 0 ? (K - (N - 1)) : 0;
  constexpr int HI = (K - 1) / 2;
  constexpr int M = HI - LO + 1;
  if constexpr (M >= 1) {
    u32 pa[M], pb[M];
#pragma unroll
    for (int m = 0; m < M; m++) { pa[m] = a[LO + m]; pb[m] = a[K - LO - m]; }
    if constexpr (SPEC && M == 1 && sqr_cross_first_nc<N>(K)) mac_nc(c, pa[0], pb[0]);     // plain C++: a three-address mad, c.hi stays zero
    else if constexpr (SPEC && M >= 2 && sqr_cross_first_nc<N>(K)) mac_cols<M, true, 1>(c, pa, pb);
    else mac_cols<M, true, 0, (SPEC && M >= 2)>(c, pa, pb, raised);
  }
}
template <int N, int K, bool SPEC>
ECGPU_HD void sqr_cross_columns(u32* x, Acc96& c, const u32* a, u64& raised) {
  if constexpr (K < 2 * N - 2) {
    u64 k = 0;
    mac_cross_column<N, K, SPEC>(c, a, k);
    if constexpr (SPEC && (K - 1) / 2 - ((K - (N - 1)) > 0 ? (K - (N - 1)) : 0) + 1 >= 2 && !sqr_cross_first_nc<N>(K)) { ECGPU_SPEC_NOTE("sqr", K, k != 0); }
    raised |= k;
    x[K] = acc_pop(c);
    sqr_cross_columns<N, K + 1, SPEC>(x, c, a, raised);
  }
}

// r[0..2N) = a * a : off-diagonal products once, doubled by a one-bit funnel shift, plus the squares
template <int N>
ECGPU_HD void mp_sqr_wide(u32* r, const u32* a) {
  u32 x[2 * N];
  Acc96 c{0, 0};
  x[0] = 0;
  sqr_cross_columns<N, 1>(x, c, a);
  x[2 * N - 2] = (u32)c.lo;   // the cross sum is < 2^(64N-1): it fits, top bit clear
  x[2 * N - 1] = (u32)(c.lo >> 32);
  // r = 2*x + sum a_i^2 2^(64 i)
  u32 carry = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const u64 d = (u64)a[i] * a[i];
    const u32 lo2 = (x[2 * i] << 1) | (i ? (x[2 * i - 1] >> 31) : 0);
    const u32 hi2 = (x[2 * i + 1] << 1) | (x[2 * i] >> 31);
    r[2 * i] = addc(lo2, (u32)d, carry);
    r[2 * i + 1] = addc(hi2, (u32)(d >> 32), carry);
  }
}
// the same with speculative cross columns (SPEC); `raised` collects their flags
template <int N, bool SPEC>
ECGPU_HD void mp_sqr_wide(u32* r, const u32* a, u64& raised) {
  u32 x[2 * N];
  Acc96 c{0, 0};
  x[0] = 0;
  sqr_cross_columns<N, 1, SPEC>(x, c, a, raised);
  x[2 * N - 2] = (u32)c.lo;   // the cross sum is < 2^(64N-1): it fits, top bit clear
  x[2 * N - 1] = (u32)(c.lo >> 32);
  // r = 2*x + sum a_i^2 2^(64 i)
  u32 carry = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const u64 d = (u64)a[i] * a[i];
    const u32 lo2 = (x[2 * i] << 1) | (i ? (x[2 * i - 1] >> 31) : 0);
    const u32 hi2 = (x[2 * i + 1] << 1) | (x[2 * i] >> 31);
    r[2 * i] = addc(lo2, (u32)d, carry);
    r[2 * i + 1] = addc(hi2, (u32)(d >> 32), carry);
  }
}

// byte order helpers: canonical wire format is big-endian (to_bytes / to_repr of the reference)
ECGPU_HD u32 bswap32(u32 x) { return __builtin_bswap32(x); }

}  // namespace ecgpu
