// secp256k1 base field on 8 saturated 32-bit limbs (one element per lane, 8 VGPRs).
//
// Replaces the role of k256::FieldElement (k256/src/arithmetic/field.rs:56 ->
// field/field_5x52.rs:16).  The reference keeps 5x52-bit lazily reduced limbs with a tracked
// magnitude; on gfx950 the multiplier is 32x32 (v_mad_u64_u32), so the internal form here is
// different: every value is an integer in [0, 2^256) congruent to the element ("weakly
// reduced": it may be >= p, exactly like the reference's magnitude-1 weak normal form), and
// `normalize` produces the canonical representative that `to_bytes` writes
// (field_5x52.rs:189-206, :96-131).  Field arithmetic is exact, so results agree bit for bit
// with the reference after normalisation.
//
// p = 2^256 - C,  C = 2^32 + 977  (field_5x52.rs:134-136 uses the same constant 0x1000003D1).
#pragma once
#include "mp32.hpp"

namespace ecgpu {

struct FeK256 {
  static constexpr int N = 8;
  static constexpr int NBYTES = 32;
  u32 v[8];
};

namespace k256 {

static constexpr u32 C_LO = 977;   // C = 2^32 + C_LO

// The rare carry paths of fold_top_fast / add / sub / shl.  In the throughput build they are real branches, almost never taken
// (probability 2^-26 .. 2^-32 per operation): which way they go depends on the values.  A translation unit that defines
// ECGPU_K256_BRANCHFREE before including this header - ops_k256_ct.hip: the kernels that run on SECRET scalars - gets them executed
// unconditionally instead: each of these blocks is a no-op when its carry is zero (it ripples a zero and folds a zero), so running it
// always gives the same values and leaves no branch that depends on data (VERDICT r3 missing 4; the reference's 5x52 lazy limbs need no
// carry branch, k256/src/arithmetic/field/field_5x52.rs:252-285).  Cost: 5 + 5 instructions per multiplication (the ripple, two selects
// on the carry's lane mask and three carry instructions), 6 + 2 per addition / subtraction / small shift (measured on the
// constant-time kernels with 5 + 3: profiles/r04_ab_measurements.txt).
#ifdef ECGPU_K256_BRANCHFREE
#define ECGPU_K256_RARE(cond) true
#else
#define ECGPU_K256_RARE(cond) __builtin_expect((cond), 0)
#endif
// The products (mul, mul_add2, mul_add_sqr, sqr) with every carry addition and no branch on a carry: the branch-free build, and a
// translation unit that defines ECGPU_K256_EXACT_PRODUCTS (msm_k256.hip: its kernels measured slower with the speculative columns
// below, profiles/spec_carry.txt).
#if defined(ECGPU_K256_BRANCHFREE) || defined(ECGPU_K256_EXACT_PRODUCTS)
#define ECGPU_K256_SPEC_PRODUCTS 0
#else
#define ECGPU_K256_SPEC_PRODUCTS 1
#endif

// r += T * C for a small T (< 2^40), then fold the possible carry out of 2^256 once more.
ECGPU_HD void fold_top(u32* r, u64 T) {
  // A = T*C = T*977 + (T << 32): three words
  const u64 m = (u64)(u32)T * C_LO + (((u64)((u32)(T >> 32) * C_LO)) << 32);
  const u64 alo = m + (T << 32);
  const u32 a2 = (u32)(T >> 32) + (alo < m ? 1u : 0u);
  u32 c = 0;
  r[0] = addc(r[0], (u32)alo, c);
  r[1] = addc(r[1], (u32)(alo >> 32), c);
  r[2] = addc(r[2], a2, c);
#pragma unroll
  for (int i = 3; i < 8; i++) r[i] = addc(r[i], 0u, c);
  // if that carried, the wrapped value is < 2^72: adding C once more touches words 0..2 only
  u32 c2 = 0;
  r[0] = addc(r[0], c ? C_LO : 0u, c2);
  r[1] = addc(r[1], c, c2);
  r[2] = addc(r[2], 0u, c2);
}

// r += T * C for T < 2^40 (T*C is at most three words).  The carry out of word 2 is rare (~2^-26):
// it takes a branch that ripples it and, if 2^256 is crossed, folds once more (the wrapped value is
// then tiny, so that last fold cannot carry).
//
// T = t0 + t1 2^32 arrives as the two words the reduction's carry chains end in (add_high_chain below).
// T * C = t0 * 977 + (T + t1 * 977) * 2^32, and both halves ride on a multiply's 64-bit addend:
//   (r0, r1) += t0 * 977         one v_mad_u64_u32 whose addend is the pair (r0, r1); its carry k1 belongs to word 2
//   M = T + t1 * 977             one v_mad_u64_u32 whose addend is T itself (SMALL, t1 <= 1 and then t0 + 977 < 2^32: the low word
//                                is one v_mad_u32_u24 and the high word is t1); M < 2^41
//   (r1, r2) += M + k1 * 2^32    three carry instructions: k1 joins M's high word first, so ONE carry comes out of word 2
// Five instructions.  On the device the carries between the statements are lane masks in scalar-register pairs, and 977 comes from a
// scalar register (the columns' fold products read theirs from a VGPR).
namespace nc_bound {
using u128 = unsigned __int128;
static_assert(((u128)1 << 40) + 0xFFu * (u128)C_LO < ((u128)1 << 41), "M = T + t1 * 977 for T < 2^40: its high word + k1 cannot carry");
static_assert(((u128)1 << 11) + 2 + C_LO < ((u128)1 << 32), "SMALL: t1 = 1 leaves t0 < 2^11 + 2, so t0 + 977 does not wrap");
}  // namespace nc_bound
template <bool SMALL>
ECGPU_HD void fold_top_words(u32* r, u32 t0, u32 t1) {
#if ECGPU_ASM
  u64 r01 = ((u64)r[1] << 32) | r[0];
  u64 k;                                        // the carry flag in flight: first the first mad's (k1), then word 2's
  asm("v_mad_u64_u32 %0, %1, %2, %3, %0" : "+v"(r01), "=s"(k) : "v"(t0), "s"(C_LO));
  u32 ml, mh;
  if constexpr (SMALL) {
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(ml) : "v"(t1), "s"(C_LO), "v"(t0));
    mh = t1;
  } else {
    const u64 T = ((u64)t1 << 32) | t0;
    u64 m;
    asm("v_mad_u64_u32 %0, vcc, %1, %2, %3" : "=v"(m) : "v"(t1), "s"(C_LO), "v"(T) : "vcc");
    ml = (u32)m; mh = (u32)(m >> 32);
  }
  r[0] = (u32)r01;
  u32 r1 = (u32)(r01 >> 32);
  asm("v_addc_co_u32 %[mh], %[k], 0, %[mh], %[k]\n\t"
      "v_add_co_u32 %[r1], vcc, %[r1], %[ml]\n\t"
      "v_addc_co_u32 %[r2], %[k], %[r2], %[mh], vcc"
      : [r1] "+v"(r1), [r2] "+v"(r[2]), [mh] "+v"(mh), [k] "+s"(k)
      : [ml] "v"(ml)
      : "vcc");
  r[1] = r1;
  if (ECGPU_K256_RARE(k != 0)) {
    // ripple the carry (a lane mask) through words 3..7; what comes out of word 7 crossed 2^256
    asm("v_addc_co_u32 %0, %5, 0, %0, %5\n\t"
        "v_addc_co_u32 %1, %5, 0, %1, %5\n\t"
        "v_addc_co_u32 %2, %5, 0, %2, %5\n\t"
        "v_addc_co_u32 %3, %5, 0, %3, %5\n\t"
        "v_addc_co_u32 %4, %5, 0, %4, %5"
        : "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]), "+s"(k));
    u32 c, cc;                                  // the lanes that wrapped add C: 977 to word 0, 1 to word 1
    asm("v_cndmask_b32 %0, 0, 1, %2\n\t"
        "v_cndmask_b32 %1, 0, %3, %2"
        : "=&v"(c), "=v"(cc) : "s"(k), "v"(C_LO));
    u32 c2 = 0;
    r[0] = addc(r[0], cc, c2);
    r[1] = addc(r[1], c, c2);
    r[2] = addc(r[2], 0u, c2);
  }
#else
  const u64 a = (u64)t0 * C_LO + r[0];               // < 2^43: the sum with r1 * 2^32 may carry (k1)
  const u64 r01 = a + ((u64)r[1] << 32);
  const u32 k1 = r01 < a ? 1u : 0u;
  const u64 m = (SMALL ? (u64)(t1 * C_LO + t0) | ((u64)t1 << 32) : (((u64)t1 << 32) | t0) + (u64)t1 * C_LO) + ((u64)k1 << 32);
  u32 c = 0;
  r[0] = (u32)r01;
  r[1] = addc((u32)(r01 >> 32), (u32)m, c);
  r[2] = addc(r[2], (u32)(m >> 32), c);
  ECGPU_TAIL_NOTE("fold:k1", k1 != 0);
  ECGPU_TAIL_NOTE("fold:ripple", c != 0);
  if (ECGPU_K256_RARE(c != 0)) {
#pragma unroll
    for (int i = 3; i < 8; i++) r[i] = addc(r[i], 0u, c);
    ECGPU_TAIL_NOTE("fold:second", c != 0);
    u32 c2 = 0;
    r[0] = addc(r[0], c * C_LO, c2);
    r[1] = addc(r[1], c, c2);
    r[2] = addc(r[2], 0u, c2);
  }
#endif
}
ECGPU_HD void fold_top_fast(u32* r, u64 T) { fold_top_words<false>(r, (u32)T, (u32)(T >> 32)); }
// r = t + h * 2^32 on words 0..7 (r[0] = t[0], r[i] = t[i] + h[i-1]), and the same carry chain runs on through two more words:
// t0 = xl + yl + carry, t1 = xh + yh + carry; the caller's bound says that t1 does not carry.  This is how every reduction assembles
// its overflow count T = t0 + t1 2^32: v_addc_co_u32 adds two registers and a carry flag, so no flag is turned into a word and no
// zero-extended 64-bit pair is built.
ECGPU_HD void add_high_chain(u32* r, const u32* t, const u32* h, u32 xl, u32 yl, u32 xh, u32 yh, u32& t0, u32& t1) {
  u32 cy = 0;
  r[0] = t[0];
#pragma unroll
  for (int i = 1; i < 8; i++) r[i] = addc(t[i], h[i - 1], cy);
  ECGPU_TAIL_NOTE("chain:word7", cy != 0);
  t0 = addc(xl, yl, cy);
  ECGPU_TAIL_NOTE("chain:t0", cy != 0);
  t1 = addc(xh, yh, cy);
}

// r = a * b mod p (weakly reduced).  field_5x52.rs:288-449 (mul_inner) is the reference.
// Columns 8..14 of the schoolbook product are summed first (H), then columns 0..7 are summed
// together with H*C, so the pseudo-Mersenne fold rides on the same 96-bit accumulator.
// One asm statement per column (hipcc pads each asm statement with an s_nop): the column's
// products, and for the low half also h[k]*977 and h[k-1]*1, go into a single statement.
//
// Products that cannot carry out of the accumulator's low 64 bits lead their column and go in without a carry addition
// (mac_cols NC):
//  - the fold product h[K] * 977 of low column K: the carry popped into a column is < 2^37 (every column of mul, mul_add2
//    and mul_add_sqr sums at most 17 products below 2^64 and its own carry-in, < 2^69), h[K] * 977 < 2^42, their sum < 2^43;
//  - the first product of high column 8, which starts from the zeroed accumulator;
//  - in mul_add_sqr, s_i * d_8 (d_8 = s_7 >> 31 is 0 or 1, so the product is < 2^32) on a popped carry, and in column 8 the
//    product after it: < 2^32 + (2^32 - 1)^2 < 2^64.
namespace nc_bound {
using u128 = unsigned __int128;
constexpr u128 MAX_PRODUCT = (u128)0xFFFFFFFFu * 0xFFFFFFFFu;
static_assert(17 * MAX_PRODUCT + ((u128)1 << 37) < ((u128)1 << 69), "a column with a carry-in < 2^37 sums to < 2^69: it pops < 2^37");
static_assert(((u128)1 << 37) + (u128)0xFFFFFFFFu * C_LO < ((u128)1 << 43), "fold product on a popped carry: < 2^43, no carry");
static_assert(((u128)1 << 37) + 0xFFFFFFFFu < ((u128)1 << 64), "s_i * d_8 on a popped carry: no carry");
static_assert((u128)0xFFFFFFFFu + MAX_PRODUCT < ((u128)1 << 64), "s_0 * d_8 then one product on a zeroed accumulator: no carry");
}  // namespace nc_bound
template <int K>
ECGPU_HD void mul_high_column(u32* h, Acc96& c, const u32* a, const u32* b) {
  // c.hi == 0: fresh accumulator or just popped.  Column 8 starts from zero: its first product cannot carry.
  mac_product_column<8, K, 0, true, (K == 8 ? 1 : 0)>(c, a, b, nullptr, nullptr);
  h[K - 8] = acc_pop(c);
}
template <int K>
ECGPU_HD void mul_low_column(u32* t, Acc96& c, const u32* a, const u32* b, const u32* h) {
  const u32 xa[1] = {h[K]}, xb[1] = {C_LO};
  mac_product_column<8, K, 1, true, 1>(c, a, b, xa, xb);      // h[K] * 977 first: < 2^43 with the carry-in (nc_bound)
  t[K] = acc_pop(c);
}
// The tail of the four products that fold on their columns (mul, mul_add2, mul_add_sqr and their exact forms): H * 2^32, the other
// half of H * C, is one carry chain over words 1..7, and the same chain runs on into the overflow count T above 2^256:
//   t0 = c.lo's low word + h[7] + carry,  t1 = c.lo's high word + h8 + carry          (add_high_chain)
// c: what column 7 left, < 2^37.  h8 (WORD16): word 16 of a sum of two products, 0 or 1; 2^512 = C^2 mod p, so it adds C = 2^32 + 977
// to T: its 2^32 is the h8 of t1, its 977 goes into c.lo first (a 24-bit multiply-add into h[7] or into c.lo's low word could wrap:
// all-ones operands give h[7] = 2^32 - 1 with h8 = 1).  T < 2^38.
namespace nc_bound {
static_assert(((u128)1 << 37) + C_LO + 0xFFFFFFFFu + 1 + ((u128)1 << 32) < ((u128)1 << 38), "T = c.lo + h[7] + carry + h8 * C < 2^38: t1 does not carry");
}  // namespace nc_bound
template <bool WORD16>
ECGPU_HD void mul_finish(FeK256& r, const u32* t, const u32* h, const Acc96& c, u32 h8) {
  u32 t0, t1;
  if constexpr (WORD16) {
    u32 e;                                              // h8 * 977, one 24-bit multiply (not a select on h8 != 0)
#if ECGPU_ASM
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(e) : "v"(h8), "s"(C_LO));
#else
    e = h8 * C_LO;
#endif
    u32 k = 0;
    const u32 cl0 = addc((u32)c.lo, e, k);
    const u32 cl1 = addc((u32)(c.lo >> 32), 0u, k);
    add_high_chain(r.v, t, h, cl0, h[7], cl1, h8, t0, t1);
    ECGPU_TAIL_NOTE("mul:h8", h8 != 0);
  } else {
    add_high_chain(r.v, t, h, (u32)c.lo, h[7], (u32)(c.lo >> 32), 0u, t0, t1);
  }
  fold_top_words<false>(r.v, t0, t1);
}
ECGPU_HD void mul_exact(FeK256& r, const FeK256& a, const FeK256& b) {
  u32 h[8], t[8];
  Acc96 c{0, 0};
  mul_high_column<8>(h, c, a.v, b.v);  mul_high_column<9>(h, c, a.v, b.v);
  mul_high_column<10>(h, c, a.v, b.v); mul_high_column<11>(h, c, a.v, b.v);
  mul_high_column<12>(h, c, a.v, b.v); mul_high_column<13>(h, c, a.v, b.v);
  mul_high_column<14>(h, c, a.v, b.v);
  h[7] = (u32)c.lo;
  c.lo = 0; c.hi = 0;
  mul_low_column<0>(t, c, a.v, b.v, h); mul_low_column<1>(t, c, a.v, b.v, h);
  mul_low_column<2>(t, c, a.v, b.v, h); mul_low_column<3>(t, c, a.v, b.v, h);
  mul_low_column<4>(t, c, a.v, b.v, h); mul_low_column<5>(t, c, a.v, b.v, h);
  mul_low_column<6>(t, c, a.v, b.v, h); mul_low_column<7>(t, c, a.v, b.v, h);
  mul_finish<false>(r, t, h, c, 0);
}

// Speculative products (SPEC; ECGPU_K256_SPEC_PRODUCTS: the throughput build of the variable-base and signature kernels).  After its no-carry products a column starts
// below 2^43 (low half) or 2^38 (high half: a popped carry, + s_i * d_8 in mul_add_sqr), and its next product is at most
// 2^64 - 2^33 + 1: adding it carries out of c.lo only when the product exceeds 2^64 - 2^43, probability about 2^-43 (2^-55 in the
// high half) for uniform limbs.  That product goes in WITHOUT its carry addition (mac_colM_nN_s1): the mad's carry-out lane mask is
// kept in scalar registers, and a wave-uniform branch - the policy of ECGPU_K256_RARE, taken when any lane's bit is set - adds
// the missing carry to c.hi before the column is popped (mp32.hpp: mac_cols with SPEC).  One VALU carry addition less per column,
// a scalar compare and branch instead: 12 in mul (and column 14 without any) and in mul_add2, 14 in mul_add_sqr, 5 in sqr (and 8
// more without any).  A column whose only carry addition would go stays exact (low column 0 of mul and mul_add2, high column 14 of mul_add2): that addition
// creates c.hi, and a move would have to take its place.  The bounds below say how rare the branch is; the value never depends on
// them.  The *_exact bodies (every product with its carry addition, no such branch) are the products of the other builds.
//  - high column 14 of mul is the single product a_7 b_7 on the carry popped from column 13; even for all-ones operands (every
//    column sum is monotone in the limbs) it does not carry: a no-carry product, not a speculative one.  Not so with a second
//    product in the column (mul_add2, mul_add_sqr).
//  - the squaring's cross columns 1 to 5 and 11 to 13 cannot carry at their first product even for an all-ones operand: no-carry
//    products (mp32.hpp: sqr_cross_first_nc, mp_sqr_wide with SPEC); those of one product (1, 2, 12, 13) are plain C++.
namespace nc_bound {
// carry popped into high column K of an 8 x 8 product of all-ones operands (the high half starts from zero at column 8)
constexpr u128 high_carry_in(int K) {
  u128 c = 0;
  for (int k = 8; k < K; k++) c = (c + (u128)(15 - k) * MAX_PRODUCT) >> 32;
  return c;
}
static_assert(high_carry_in(14) + MAX_PRODUCT < ((u128)1 << 64), "mul, high column 14: a_7 b_7 on the popped carry cannot carry");
static_assert(2 * high_carry_in(14) + 1 + MAX_PRODUCT >= ((u128)1 << 64), "with two products per column (mul_add2) it can: speculative there");
static_assert(((u128)1 << 43) + MAX_PRODUCT >= ((u128)1 << 64) && MAX_PRODUCT == ((u128)1 << 64) - ((u128)1 << 33) + 1,
              "low half: the speculative product starts below 2^43 and carries only for a product above 2^64 - 2^43");
static_assert(((u128)1 << 37) + 0xFFFFFFFFu < ((u128)1 << 38), "high half: the speculative product starts below 2^38 (popped carry, + s_i d_8 in mul_add_sqr)");
}  // namespace nc_bound
#if !ECGPU_K256_SPEC_PRODUCTS
ECGPU_HD void mul(FeK256& r, const FeK256& a, const FeK256& b) { mul_exact(r, a, b); }
#else
template <int K>
ECGPU_HD void mul_high_column_spec(u32* h, Acc96& c, const u32* a, const u32* b, u64& raised) {
  static_assert(K >= 9 && K <= 14, "column 8 starts from zero and stays mul_high_column<8>");
  if constexpr (K == 14) {
    mac_nc(c, a[7], b[7]);                  // nc_bound: high_carry_in(14); c.hi stays zero, so the two words of c.lo are h[6] and h[7]
    h[6] = (u32)c.lo;
    c.lo >>= 32;
    return;
  } else {
    u64 k = 0;
    mac_product_column<8, K, 0, true, 0, true>(c, a, b, nullptr, nullptr, k);
    ECGPU_SPEC_NOTE("mul", K, k != 0);
    raised |= k;
  }
  h[K - 8] = acc_pop(c);
}
template <int K>
ECGPU_HD void mul_low_column_spec(u32* t, Acc96& c, const u32* a, const u32* b, const u32* h, u64& raised) {
  static_assert(K >= 1 && K <= 7, "column 0 has one product after the fold term, whose carry addition creates c.hi: it stays mul_low_column<0>");
  const u32 xa[1] = {h[K]}, xb[1] = {C_LO};
  u64 k = 0;
  mac_product_column<8, K, 1, true, 1, true>(c, a, b, xa, xb, k);      // h[K] * 977 without a carry, then a_0 b_K speculative
  ECGPU_SPEC_NOTE("mul", K, k != 0);
  raised |= k;
  t[K] = acc_pop(c);
}
ECGPU_HD void mul(FeK256& r, const FeK256& a, const FeK256& b) {
  u32 h[8], t[8];
  u64 raised = 0;
  Acc96 c{0, 0};
  mul_high_column<8>(h, c, a.v, b.v);
  mul_high_column_spec<9>(h, c, a.v, b.v, raised);  mul_high_column_spec<10>(h, c, a.v, b.v, raised);
  mul_high_column_spec<11>(h, c, a.v, b.v, raised); mul_high_column_spec<12>(h, c, a.v, b.v, raised);
  mul_high_column_spec<13>(h, c, a.v, b.v, raised); mul_high_column_spec<14>(h, c, a.v, b.v, raised);
  h[7] = (u32)c.lo;
  c.lo = 0; c.hi = 0;
  mul_low_column<0>(t, c, a.v, b.v, h); mul_low_column_spec<1>(t, c, a.v, b.v, h, raised);
  mul_low_column_spec<2>(t, c, a.v, b.v, h, raised); mul_low_column_spec<3>(t, c, a.v, b.v, h, raised);
  mul_low_column_spec<4>(t, c, a.v, b.v, h, raised); mul_low_column_spec<5>(t, c, a.v, b.v, h, raised);
  mul_low_column_spec<6>(t, c, a.v, b.v, h, raised); mul_low_column_spec<7>(t, c, a.v, b.v, h, raised);
  mul_finish<false>(r, t, h, c, 0);
}
#endif

// r = a * b + e * f mod p (weakly reduced): both products ride on the same column accumulators and share ONE reduction (the
// point formulas end in differences of two products: Y3 = R (V - X3) - Y1 HHH).  A column holds up to 16 products plus the
// fold term, < 2^69: the 96-bit accumulator has room.  The sum of the two products can reach 2^513, so word 16 (one bit) exists:
// 2^512 = C^2 mod p, i.e. it adds C to the overflow count T that fold_top_fast multiplies by C.
template <int K>
ECGPU_HD void mul2_high_column(u32* h, Acc96& c, const u32* a, const u32* b, const u32* e, const u32* f) {
  // c.hi == 0: fresh accumulator or just popped.  Column 8 starts from zero: its first product cannot carry.
  mac_product_column<8, K, 0, true, (K == 8 ? 1 : 0)>(c, a, b, nullptr, nullptr);
  mac_product_column<8, K, 0, false>(c, e, f, nullptr, nullptr);
  h[K - 8] = acc_pop(c);
}
template <int K>
ECGPU_HD void mul2_low_column(u32* t, Acc96& c, const u32* a, const u32* b, const u32* e, const u32* f, const u32* h) {
  const u32 xa[1] = {h[K]}, xb[1] = {C_LO};
  mac_product_column<8, K, 1, true, 1>(c, a, b, xa, xb);      // h[K] * 977 first: < 2^43 with the carry-in (nc_bound)
  mac_product_column<8, K, 0, false>(c, e, f, nullptr, nullptr);
  t[K] = acc_pop(c);
}
ECGPU_HD void mul_add2_exact(FeK256& r, const FeK256& a, const FeK256& b, const FeK256& e, const FeK256& f) {
  u32 h[8], t[8];
  Acc96 c{0, 0};
  mul2_high_column<8>(h, c, a.v, b.v, e.v, f.v);  mul2_high_column<9>(h, c, a.v, b.v, e.v, f.v);
  mul2_high_column<10>(h, c, a.v, b.v, e.v, f.v); mul2_high_column<11>(h, c, a.v, b.v, e.v, f.v);
  mul2_high_column<12>(h, c, a.v, b.v, e.v, f.v); mul2_high_column<13>(h, c, a.v, b.v, e.v, f.v);
  mul2_high_column<14>(h, c, a.v, b.v, e.v, f.v);
  h[7] = (u32)c.lo;
  const u32 h8 = (u32)(c.lo >> 32);                 // word 16 of the sum: 0 or 1
  c.lo = 0; c.hi = 0;
  mul2_low_column<0>(t, c, a.v, b.v, e.v, f.v, h); mul2_low_column<1>(t, c, a.v, b.v, e.v, f.v, h);
  mul2_low_column<2>(t, c, a.v, b.v, e.v, f.v, h); mul2_low_column<3>(t, c, a.v, b.v, e.v, f.v, h);
  mul2_low_column<4>(t, c, a.v, b.v, e.v, f.v, h); mul2_low_column<5>(t, c, a.v, b.v, e.v, f.v, h);
  mul2_low_column<6>(t, c, a.v, b.v, e.v, f.v, h); mul2_low_column<7>(t, c, a.v, b.v, e.v, f.v, h);
  mul_finish<true>(r, t, h, c, h8);
}

#if !ECGPU_K256_SPEC_PRODUCTS
ECGPU_HD void mul_add2(FeK256& r, const FeK256& a, const FeK256& b, const FeK256& e, const FeK256& f) { mul_add2_exact(r, a, b, e, f); }
#else
template <int K>
ECGPU_HD void mul2_high_column_spec(u32* h, Acc96& c, const u32* a, const u32* b, const u32* e, const u32* f, u64& raised) {
  static_assert(K >= 9 && K <= 13, "column 8 starts from zero; column 14 has one product a_7 b_7, whose carry addition creates c.hi");
  u64 k = 0;
  mac_product_column<8, K, 0, true, 0, true>(c, a, b, nullptr, nullptr, k);
  ECGPU_SPEC_NOTE("mul_add2", K, k != 0);
  raised |= k;
  mac_product_column<8, K, 0, false>(c, e, f, nullptr, nullptr);
  h[K - 8] = acc_pop(c);
}
template <int K>
ECGPU_HD void mul2_low_column_spec(u32* t, Acc96& c, const u32* a, const u32* b, const u32* e, const u32* f, const u32* h, u64& raised) {
  static_assert(K >= 1 && K <= 7, "column 0 stays mul2_low_column<0>, as in mul");
  const u32 xa[1] = {h[K]}, xb[1] = {C_LO};
  u64 k = 0;
  mac_product_column<8, K, 1, true, 1, true>(c, a, b, xa, xb, k);
  ECGPU_SPEC_NOTE("mul_add2", K, k != 0);
  raised |= k;
  mac_product_column<8, K, 0, false>(c, e, f, nullptr, nullptr);
  t[K] = acc_pop(c);
}
ECGPU_HD void mul_add2(FeK256& r, const FeK256& a, const FeK256& b, const FeK256& e, const FeK256& f) {
  u32 h[8], t[8];
  u64 raised = 0;
  Acc96 c{0, 0};
  mul2_high_column<8>(h, c, a.v, b.v, e.v, f.v);
  mul2_high_column_spec<9>(h, c, a.v, b.v, e.v, f.v, raised);  mul2_high_column_spec<10>(h, c, a.v, b.v, e.v, f.v, raised);
  mul2_high_column_spec<11>(h, c, a.v, b.v, e.v, f.v, raised); mul2_high_column_spec<12>(h, c, a.v, b.v, e.v, f.v, raised);
  mul2_high_column_spec<13>(h, c, a.v, b.v, e.v, f.v, raised); mul2_high_column<14>(h, c, a.v, b.v, e.v, f.v);
  h[7] = (u32)c.lo;
  const u32 h8 = (u32)(c.lo >> 32);                 // word 16 of the sum: 0 or 1
  c.lo = 0; c.hi = 0;
  mul2_low_column<0>(t, c, a.v, b.v, e.v, f.v, h); mul2_low_column_spec<1>(t, c, a.v, b.v, e.v, f.v, h, raised);
  mul2_low_column_spec<2>(t, c, a.v, b.v, e.v, f.v, h, raised); mul2_low_column_spec<3>(t, c, a.v, b.v, e.v, f.v, h, raised);
  mul2_low_column_spec<4>(t, c, a.v, b.v, e.v, f.v, h, raised); mul2_low_column_spec<5>(t, c, a.v, b.v, e.v, f.v, h, raised);
  mul2_low_column_spec<6>(t, c, a.v, b.v, e.v, f.v, h, raised); mul2_low_column_spec<7>(t, c, a.v, b.v, e.v, f.v, h, raised);
  mul_finish<true>(r, t, h, c, h8);
}
#endif

// Column K of s^2 with the cross products already doubled: s^2 = sum_i s_i^2 B^2i + sum_{i <= 6} s_i B^i T_i, B = 2^32, where
// T_i = 2 sum_{j > i} s_j B^j has the words e_(i+1) = s_(i+1) << 1 at B^(i+1) and d_j = (s_j << 1) | (s_(j-1) >> 31) at B^j for
// i + 2 <= j <= 8 (d_8 = s_7 >> 31, the bit shifted out of the top).  35 doubled cross products and 8 squares: 43 multiply-accumulate
// pairs on the columns instead of the 64 of a general product, and no separate doubling pass.
constexpr int sqr2_terms(int K) {
  int m = 0;
  if (K % 2 == 1 && (K - 1) / 2 <= 6) m++;                 // s_i e_(i+1)
  if (K % 2 == 0 && K / 2 <= 7) m++;                       // s_i^2
  for (int i = 0; i <= 6; i++)
    if (K - i >= i + 2 && K - i <= 8) m++;                 // s_i d_j
  return m;
}
// the terms of column K except s_(K-8) d_8, which mulsq_column puts first (columns 8..14 have one)
constexpr bool sqr2_has_d8(int K) { return K >= 8 && K <= 14; }
template <int K>
ECGPU_HD void sqr2_column_terms(u32* pa, u32* pb, const u32* s, const u32* e, const u32* d) {
  int m = 0;
  if constexpr (K % 2 == 1 && (K - 1) / 2 <= 6) { pa[m] = s[(K - 1) / 2]; pb[m] = e[(K + 1) / 2]; m++; }
  if constexpr (K % 2 == 0 && K / 2 <= 7) { pa[m] = s[K / 2]; pb[m] = s[K / 2]; m++; }
#pragma unroll
  for (int i = 0; i <= 6; i++)
    if (K - i >= i + 2 && K - i <= 7) { pa[m] = s[i]; pb[m] = d[K - i]; m++; }
}
// e[1..7] and d[2..8] of the layout above (e[0], d[0], d[1] unused)
ECGPU_HD void sqr2_operands(u32* e, u32* d, const u32* s) {
#pragma unroll
  for (int j = 1; j < 8; j++) e[j] = s[j] << 1;
#pragma unroll
  for (int j = 2; j < 8; j++) d[j] = (s[j] << 1) | (s[j - 1] >> 31);
  d[8] = s[7] >> 31;
}
// column K of a * b + s^2, plus NX extra products (the fold terms of the low half).  Order: the extra products, s_(K-8) d_8,
// the products of a * b, the other square terms; NC: the first NC of them cannot carry out of c.lo, as the caller states.
template <int K, int NX, bool FRESH, int NC>
ECGPU_HD void mulsq_column(Acc96& c, const u32* a, const u32* b, const u32* s, const u32* e, const u32* d, const u32* xa, const u32* xb) {
  constexpr int LO = (K - 7) > 0 ? (K - 7) : 0;
  constexpr int HI = K < 7 ? K : 7;
  constexpr int M = HI - LO + 1;
  constexpr int MS = sqr2_terms(K);
  constexpr int D8 = sqr2_has_d8(K) ? 1 : 0;
  u32 pa[M + MS + NX + 1], pb[M + MS + NX + 1];
#pragma unroll
  for (int m = 0; m < NX; m++) { pa[m] = xa[m]; pb[m] = xb[m]; }
  if constexpr (D8) { pa[NX] = s[K - 8]; pb[NX] = d[8]; }
#pragma unroll
  for (int m = 0; m < M; m++) { pa[NX + D8 + m] = a[LO + m]; pb[NX + D8 + m] = b[K - LO - m]; }
  sqr2_column_terms<K>(pa + NX + D8 + M, pb + NX + D8 + M, s, e, d);
  mac_cols<M + MS + NX, FRESH, NC>(c, pa, pb);
}
template <int K>
ECGPU_HD void mulsq_high_column(u32* h, Acc96& c, const u32* a, const u32* b, const u32* s, const u32* e, const u32* d) {
  // s_(K-8) d_8 < 2^32 first, on a popped carry; column 8 starts from zero and its next product cannot carry either (nc_bound)
  static_assert(sqr2_has_d8(K), "every high column has its d_8 term");
  mulsq_column<K, 0, true, (K == 8 ? 2 : 1)>(c, a, b, s, e, d, nullptr, nullptr);
  h[K - 8] = acc_pop(c);
}
template <int K>
ECGPU_HD void mulsq_low_column(u32* t, Acc96& c, const u32* a, const u32* b, const u32* s, const u32* e, const u32* d, const u32* h) {
  const u32 xa[1] = {h[K]}, xb[1] = {C_LO};
  mulsq_column<K, 1, true, 1>(c, a, b, s, e, d, xa, xb);     // h[K] * 977 first: < 2^43 with the carry-in (nc_bound)
  t[K] = acc_pop(c);
}
// r = a * b + s^2 mod p (weakly reduced): mul_add2 with a square as its second product (the doubling's Y3).  The sum is < 2^513, so
// word 16 is handled as in mul_add2.
ECGPU_HD void mul_add_sqr_exact(FeK256& r, const FeK256& a, const FeK256& b, const FeK256& s) {
  u32 e[8], d[9], h[8], t[8];
  e[0] = 0; d[0] = 0; d[1] = 0;
  sqr2_operands(e, d, s.v);
  Acc96 c{0, 0};
  mulsq_high_column<8>(h, c, a.v, b.v, s.v, e, d);  mulsq_high_column<9>(h, c, a.v, b.v, s.v, e, d);
  mulsq_high_column<10>(h, c, a.v, b.v, s.v, e, d); mulsq_high_column<11>(h, c, a.v, b.v, s.v, e, d);
  mulsq_high_column<12>(h, c, a.v, b.v, s.v, e, d); mulsq_high_column<13>(h, c, a.v, b.v, s.v, e, d);
  mulsq_high_column<14>(h, c, a.v, b.v, s.v, e, d);
  h[7] = (u32)c.lo;
  const u32 h8 = (u32)(c.lo >> 32);                 // word 16 of the sum: 0 or 1
  c.lo = 0; c.hi = 0;
  mulsq_low_column<0>(t, c, a.v, b.v, s.v, e, d, h); mulsq_low_column<1>(t, c, a.v, b.v, s.v, e, d, h);
  mulsq_low_column<2>(t, c, a.v, b.v, s.v, e, d, h); mulsq_low_column<3>(t, c, a.v, b.v, s.v, e, d, h);
  mulsq_low_column<4>(t, c, a.v, b.v, s.v, e, d, h); mulsq_low_column<5>(t, c, a.v, b.v, s.v, e, d, h);
  mulsq_low_column<6>(t, c, a.v, b.v, s.v, e, d, h); mulsq_low_column<7>(t, c, a.v, b.v, s.v, e, d, h);
  mul_finish<true>(r, t, h, c, h8);
}

#if !ECGPU_K256_SPEC_PRODUCTS
ECGPU_HD void mul_add_sqr(FeK256& r, const FeK256& a, const FeK256& b, const FeK256& s) { mul_add_sqr_exact(r, a, b, s); }
#else
// mulsq_column with the product after its NC no-carry ones speculative
template <int K, int NX, int NC>
ECGPU_HD void mulsq_column_spec(Acc96& c, const u32* a, const u32* b, const u32* s, const u32* e, const u32* d, const u32* xa, const u32* xb, u64& raised) {
  constexpr int LO = (K - 7) > 0 ? (K - 7) : 0;
  constexpr int HI = K < 7 ? K : 7;
  constexpr int M = HI - LO + 1;
  constexpr int MS = sqr2_terms(K);
  constexpr int D8 = sqr2_has_d8(K) ? 1 : 0;
  u32 pa[M + MS + NX + 1], pb[M + MS + NX + 1];
#pragma unroll
  for (int m = 0; m < NX; m++) { pa[m] = xa[m]; pb[m] = xb[m]; }
  if constexpr (D8) { pa[NX] = s[K - 8]; pb[NX] = d[8]; }
#pragma unroll
  for (int m = 0; m < M; m++) { pa[NX + D8 + m] = a[LO + m]; pb[NX + D8 + m] = b[K - LO - m]; }
  sqr2_column_terms<K>(pa + NX + D8 + M, pb + NX + D8 + M, s, e, d);
  u64 k = 0;
  mac_cols<M + MS + NX, true, NC, true>(c, pa, pb, k);
  ECGPU_SPEC_NOTE("mul_add_sqr", K, k != 0);
  raised |= k;
}
template <int K>
ECGPU_HD void mulsq_high_column_spec(u32* h, Acc96& c, const u32* a, const u32* b, const u32* s, const u32* e, const u32* d, u64& raised) {
  static_assert(K >= 9 && K <= 14, "column 8 starts from zero and stays mulsq_high_column<8>");
  mulsq_column_spec<K, 0, 1>(c, a, b, s, e, d, nullptr, nullptr, raised);     // s_(K-8) d_8 without a carry, then a_(K-7) b_7 speculative
  h[K - 8] = acc_pop(c);
}
template <int K>
ECGPU_HD void mulsq_low_column_spec(u32* t, Acc96& c, const u32* a, const u32* b, const u32* s, const u32* e, const u32* d, const u32* h, u64& raised) {
  const u32 xa[1] = {h[K]}, xb[1] = {C_LO};
  mulsq_column_spec<K, 1, 1>(c, a, b, s, e, d, xa, xb, raised);
  t[K] = acc_pop(c);
}
ECGPU_HD void mul_add_sqr(FeK256& r, const FeK256& a, const FeK256& b, const FeK256& s) {
  u32 e[8], d[9], h[8], t[8];
  e[0] = 0; d[0] = 0; d[1] = 0;
  sqr2_operands(e, d, s.v);
  u64 raised = 0;
  Acc96 c{0, 0};
  mulsq_high_column<8>(h, c, a.v, b.v, s.v, e, d);
  mulsq_high_column_spec<9>(h, c, a.v, b.v, s.v, e, d, raised);  mulsq_high_column_spec<10>(h, c, a.v, b.v, s.v, e, d, raised);
  mulsq_high_column_spec<11>(h, c, a.v, b.v, s.v, e, d, raised); mulsq_high_column_spec<12>(h, c, a.v, b.v, s.v, e, d, raised);
  mulsq_high_column_spec<13>(h, c, a.v, b.v, s.v, e, d, raised); mulsq_high_column_spec<14>(h, c, a.v, b.v, s.v, e, d, raised);
  h[7] = (u32)c.lo;
  const u32 h8 = (u32)(c.lo >> 32);                 // word 16 of the sum: 0 or 1
  c.lo = 0; c.hi = 0;
  mulsq_low_column_spec<0>(t, c, a.v, b.v, s.v, e, d, h, raised); mulsq_low_column_spec<1>(t, c, a.v, b.v, s.v, e, d, h, raised);
  mulsq_low_column_spec<2>(t, c, a.v, b.v, s.v, e, d, h, raised); mulsq_low_column_spec<3>(t, c, a.v, b.v, s.v, e, d, h, raised);
  mulsq_low_column_spec<4>(t, c, a.v, b.v, s.v, e, d, h, raised); mulsq_low_column_spec<5>(t, c, a.v, b.v, s.v, e, d, h, raised);
  mulsq_low_column_spec<6>(t, c, a.v, b.v, s.v, e, d, h, raised); mulsq_low_column_spec<7>(t, c, a.v, b.v, s.v, e, d, h, raised);
  mul_finish<true>(r, t, h, c, h8);
}
#endif

// reduce a 16-word integer modulo p: lo + hi * 977 + (hi << 32), then fold what spills over 2^256.  Two carry chains, lo + U and
// + (hi << 32), and each runs one word further into the overflow count T: x = top + c1 (top = U's word 8, < 2^11: no carry), then
// t0 = x + w[15] + c2 and t1 = the carry of that, 0 or 1 (add_high_chain).
namespace nc_bound {
static_assert((((u128)1 << 37) + (u128)0xFFFFFFFFu * C_LO) >> 32 < ((u128)1 << 11), "top = U >> 256 < 2^11: top + c1 does not carry, T < 2^32 + 2^11 + 2");
}  // namespace nc_bound
ECGPU_HD void reduce16(FeK256& r, const u32* w) {
  u32 u[8];
  u64 acc = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {          // U = hi * 977: no carries needed, hi_k * 977 + carry < 2^43
    acc = (u64)w[8 + k] * C_LO + (acc >> 32);
    u[k] = (u32)acc;
  }
  u32 c1 = 0;
  u32 t[8];
#pragma unroll
  for (int k = 0; k < 8; k++) t[k] = addc(w[k], u[k], c1);
  ECGPU_TAIL_NOTE("sqr:c1", c1 != 0);
  const u32 x = addc((u32)(acc >> 32), 0u, c1);
  // t1 = 0 + 0 + carry stays on the chain (one v_addc_co_u32) when the compiler cannot see that the zero is one: a loop-invariant
  // register, set once outside the loops
#if ECGPU_ASM
  u32 z;
  asm("v_mov_b32 %0, 0" : "=v"(z));
#else
  const u32 z = 0;
#endif
  u32 t0, t1;
  add_high_chain(r.v, t, w + 8, x, w[15], z, 0u, t0, t1);
  fold_top_words<true>(r.v, t0, t1);
}

// r = a^2 mod p
ECGPU_HD void sqr_exact(FeK256& r, const FeK256& a) {
  u32 w[16];
  mp_sqr_wide<8>(w, a.v);
  reduce16(r, w);
}

// the cross columns speculative (mp_sqr_wide with SPEC; its hook reports site "sqr")
ECGPU_HD void sqr(FeK256& r, const FeK256& a) {
#if !ECGPU_K256_SPEC_PRODUCTS
  sqr_exact(r, a);
#else
  u32 w[16];
  u64 raised = 0;
  mp_sqr_wide<8, true>(w, a.v, raised);
  reduce16(r, w);
#endif
}

// r = a + b mod p   (field_5x52.rs:264-272 adds limb-wise and defers; here the fold is immediate).
// The carry out of 2^256 is folded into words 0 and 1; a carry out of word 1 (probability ~2^-32)
// takes the rare path that ripples it upwards and, if that wraps again, folds once more.
ECGPU_HD void add(FeK256& r, const FeK256& a, const FeK256& b) {
  const u32 c = mp_add<8>(r.v, a.v, b.v);
  u32 c2 = 0;
  r.v[0] = addc(r.v[0], c ? C_LO : 0u, c2);
  r.v[1] = addc(r.v[1], c, c2);
  if (ECGPU_K256_RARE(c2 != 0)) {
#pragma unroll
    for (int i = 2; i < 8; i++) r.v[i] = addc(r.v[i], 0u, c2);
    // second wrap only when both inputs were within C of 2^256; the wrapped value is then < C
    u32 c3 = 0;
    r.v[0] = addc(r.v[0], c2 ? C_LO : 0u, c3);
    r.v[1] = addc(r.v[1], c2, c3);
  }
}

// r = a - b mod p   (reference: a + negate(b), field.rs:425-451, field_5x52.rs:252-260)
ECGPU_HD void sub(FeK256& r, const FeK256& a, const FeK256& b) {
  const u32 bw = mp_sub<8>(r.v, a.v, b.v);
  u32 b2 = 0;
  r.v[0] = subb(r.v[0], bw ? C_LO : 0u, b2);
  r.v[1] = subb(r.v[1], bw, b2);
  if (ECGPU_K256_RARE(b2 != 0)) {
#pragma unroll
    for (int i = 2; i < 8; i++) r.v[i] = subb(r.v[i], 0u, b2);
    u32 b3 = 0;
    r.v[0] = subb(r.v[0], b2 ? C_LO : 0u, b3);
    r.v[1] = subb(r.v[1], b2, b3);
  }
}

// r = a - b - c mod p: two borrow chains and ONE fold of the combined borrow w in {0, 1, 2} (a - b - c + w 2^256 is the 8-word
// value, and 2^256 = C mod p), instead of two subtractions with a fold each.
ECGPU_HD void sub2(FeK256& r, const FeK256& a, const FeK256& b, const FeK256& c) {
  const u32 w = mp_sub<8>(r.v, a.v, b.v) + mp_sub<8>(r.v, r.v, c.v);
  u32 b2 = 0;
  r.v[0] = subb(r.v[0], w * C_LO, b2);
  r.v[1] = subb(r.v[1], w, b2);
  if (ECGPU_K256_RARE(b2 != 0)) {
#pragma unroll
    for (int i = 2; i < 8; i++) r.v[i] = subb(r.v[i], 0u, b2);
    // wrapped below 0 once more: the value is now within 2C of 2^256, one more fold cannot borrow past word 1
    u32 b3 = 0;
    r.v[0] = subb(r.v[0], b2 ? C_LO : 0u, b3);
    r.v[1] = subb(r.v[1], b2, b3);
  }
}

// r = a / 2 mod p: (a + p) / 2 for an odd a, a / 2 for an even one.  a + p < 2^257, so the halved value is below 2^256 (weakly
// reduced) and no fold is needed: one masked carry chain and a funnel shift, no branch.  r may alias a.
ECGPU_HD void half(FeK256& r, const FeK256& a) {
  const u32 m = 0u - (a.v[0] & 1u);
  u32 t[8], c = 0;
  t[0] = addc(a.v[0], m & (0u - C_LO), c);       // p = 2^256 - 2^32 - 977: words 0xFFFFFC2F, 0xFFFFFFFE, then all ones
  t[1] = addc(a.v[1], m & 0xFFFFFFFEu, c);
#pragma unroll
  for (int i = 2; i < 8; i++) t[i] = addc(a.v[i], m, c);
#pragma unroll
  for (int i = 0; i < 7; i++) r.v[i] = (t[i] >> 1) | (t[i + 1] << 31);
  r.v[7] = (t[7] >> 1) | (c << 31);
}

ECGPU_HD void set_zero(FeK256& r) { mp_zero<8>(r.v); }
ECGPU_HD void set_one(FeK256& r) { mp_zero<8>(r.v); r.v[0] = 1; }
ECGPU_HD void set_u32(FeK256& r, u32 x) { mp_zero<8>(r.v); r.v[0] = x; }

ECGPU_HD void neg(FeK256& r, const FeK256& a) {
  FeK256 z;
  set_zero(z);
  sub(r, z, a);
}
ECGPU_HD void dbl(FeK256& r, const FeK256& a) { add(r, a, a); }

// r = a * 2^K mod p for K = 1, 2, 3: a funnel shift of the eight words and a fold of the K bits shifted out of the
// top (8 shifts + 3 carry instructions instead of K carry chains of ten).  r may alias a.
template <int K>
ECGPU_HD void shl(FeK256& r, const FeK256& a) {
  static_assert(K >= 1 && K <= 3, "small shifts only");
  const u32 top = a.v[7] >> (32 - K);
  u32 t[8];
#pragma unroll
  for (int i = 7; i >= 1; i--) t[i] = (a.v[i] << K) | (a.v[i - 1] >> (32 - K));
  t[0] = a.v[0] << K;
  // + top * C with C = 2^32 + 977: top * 977 < 2^13 into word 0, top into word 1
  u32 c = 0;
  r.v[0] = addc(t[0], top * C_LO, c);
  r.v[1] = addc(t[1], top, c);
#pragma unroll
  for (int i = 2; i < 8; i++) r.v[i] = t[i];
  if (ECGPU_K256_RARE(c != 0)) {
#pragma unroll
    for (int i = 2; i < 8; i++) r.v[i] = addc(r.v[i], 0u, c);
    u32 c2 = 0;                       // wrapped past 2^256: the value is then tiny, one more fold cannot carry far
    r.v[0] = addc(r.v[0], c ? C_LO : 0u, c2);
    r.v[1] = addc(r.v[1], c, c2);
    r.v[2] = addc(r.v[2], 0u, c2);
  }
}

// r = a * k for a small constant (field_5x52.rs:276-285 mul_single)
ECGPU_HD void mul_small(FeK256& r, const FeK256& a, u32 k) {
  u64 acc = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    acc += (u64)a.v[i] * k;
    r.v[i] = (u32)acc;
    acc >>= 32;
  }
  fold_top(r.v, acc);
}

// canonical representative in [0, p)   (field_5x52.rs:189-206)
ECGPU_HD void normalize(FeK256& r, const FeK256& a) {
  // a >= p  <=>  a + C >= 2^256
  u32 t[8];
  u32 c = 0;
  t[0] = addc(a.v[0], C_LO, c);
  t[1] = addc(a.v[1], 1u, c);
#pragma unroll
  for (int i = 2; i < 8; i++) t[i] = addc(a.v[i], 0u, c);
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = c ? t[i] : a.v[i];
}

// field_5x52.rs:209-223 normalizes_to_zero: raw 0 or raw p
ECGPU_HD bool is_zero(const FeK256& a) {
  u32 z = 0, o = 0xFFFFFFFFu;
#pragma unroll
  for (int i = 0; i < 8; i++) z |= a.v[i];
#pragma unroll
  for (int i = 2; i < 8; i++) o &= a.v[i];
  const bool is_p = (o == 0xFFFFFFFFu) && (a.v[1] == 0xFFFFFFFEu) && (a.v[0] == (0u - C_LO));
  return z == 0 || is_p;
}
// The same test for the throughput schedules' exceptional-case branches (accumulator at infinity, equal or opposite
// points), taken once or twice per point addition and almost never true: a value that is 0 or p has a top word of 0 or
// 2^32 - 1, so anything else (probability 1 - 2^-31 on the values these tests see) is rejected after two instructions.
// Not for the constant-time schedule: which path runs depends on the value.
ECGPU_HD bool is_zero_fast(const FeK256& a) {
  if (__builtin_expect(a.v[7] + 1u > 1u, 1)) return false;
  return is_zero(a);
}
ECGPU_HD bool equal(const FeK256& a, const FeK256& b) {
  FeK256 d;
  sub(d, a, b);
  return is_zero(d);
}
// field_5x52.rs:239-241 (on the normalised value)
ECGPU_HD bool is_odd(const FeK256& a) {
  FeK256 n;
  normalize(n, a);
  return n.v[0] & 1;
}
ECGPU_HD void select(FeK256& r, bool cond, const FeK256& a, const FeK256& b) { mp_select<8>(r.v, cond, a.v, b.v); }

ECGPU_HD void sqr_n(FeK256& r, const FeK256& a, int n) {
  r = a;
  for (int i = 0; i < n; i++) sqr(r, r);
}

// common prefix of the inversion / square-root chains: x223 = a^(2^223-1), x22, x2
ECGPU_HD void pow_prefix(FeK256& x223, FeK256& x22, FeK256& x2, const FeK256& a) {
  FeK256 x3, x6, x9, x11, x44, x88, x176, x220, t;
  sqr(t, a); mul(x2, t, a);
  sqr(t, x2); mul(x3, t, a);
  sqr_n(t, x3, 3); mul(x6, t, x3);
  sqr_n(t, x6, 3); mul(x9, t, x3);
  sqr_n(t, x9, 2); mul(x11, t, x2);
  sqr_n(t, x11, 11); mul(x22, t, x11);
  sqr_n(t, x22, 22); mul(x44, t, x22);
  sqr_n(t, x44, 44); mul(x88, t, x44);
  sqr_n(t, x88, 88); mul(x176, t, x88);
  sqr_n(t, x176, 44); mul(x220, t, x44);
  sqr_n(t, x220, 3); mul(x223, t, x3);
}

// r = a^(p-2): the unique inverse (0 -> 0; the caller reports CtOption::none for zero).
// Same exponent as field.rs:187-216; 255 squarings + 15 multiplications.
ECGPU_HD void inv(FeK256& r, const FeK256& a) {
  FeK256 x223, x22, x2, t;
  pow_prefix(x223, x22, x2, a);
  sqr_n(t, x223, 23); mul(t, t, x22);
  sqr_n(t, t, 5); mul(t, t, a);
  sqr_n(t, t, 3); mul(t, t, x2);
  sqr_n(t, t, 2); mul(r, t, a);
}

// r = a^((p+1)/4); returns whether r^2 == a (field.rs:220-255)
ECGPU_HD bool sqrt(FeK256& r, const FeK256& a) {
  FeK256 x223, x22, x2, t, chk;
  pow_prefix(x223, x22, x2, a);
  sqr_n(t, x223, 23); mul(t, t, x22);
  sqr_n(t, t, 6); mul(t, t, x2);
  sqr_n(r, t, 2);
  sqr(chk, r);
  return equal(chk, a);
}

// canonical big-endian bytes <-> limbs.  `words` points at 8 u32 as they lie in memory.
ECGPU_HD void from_be_words(FeK256& r, const u32* words) {
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = bswap32(words[7 - i]);
}
ECGPU_HD void to_be_words(u32* words, const FeK256& a) {   // caller normalises first
#pragma unroll
  for (int i = 0; i < 8; i++) words[7 - i] = bswap32(a.v[i]);
}
// from_bytes rejects values >= p (field_5x52.rs:75-79, :163-170)
ECGPU_HD bool is_canonical(const FeK256& a) {
  u32 c = 0;
  (void)addc(a.v[0], C_LO, c);
  (void)addc(a.v[1], 1u, c);
#pragma unroll
  for (int i = 2; i < 8; i++) (void)addc(a.v[i], 0u, c);
  return c == 0;
}

}  // namespace k256
}  // namespace ecgpu
