// Generic kernel launchers over a curve traits class; instantiated once per curve in ops_*.hip.
#pragma once
#include "ecgpu_internal.hpp"
#include "kernels.hpp"
#include "fixedbase.hpp"
#include "ecdsa_kernels.hpp"
#include "ecdh_kernels.hpp"
#include "sec1_kernels.hpp"
#include "schnorr_kernels.hpp"
#include "schnorr_batch_kernels.hpp"
#include "signing_kernels.hpp"
#include "h2c_kernels.hpp"
#include "h2c_hash.hpp"
#include "straus.hpp"
#include "scalar_ops.hpp"
// Results per lane that share one inversion in the wide fixed-base kernels.  With only 12-16 additions per result
// the inversion's share is large: measured at 2^24 scalars, batch 16 / 32 / 64: p256 0.96 / 1.03 / 1.06, k256 1.19 /
// 1.24 / 1.25 x 10^9 per second; p384 (2^22) 282 / 280 / 279 x 10^6 (its results are 144 bytes each in the private
// segment), hence 16 there.
#ifndef FB_BATCH
#define FB_BATCH (C::NW > 8 ? 16 : 64)
#endif
// results per lane a wave of the wide fixed-base kernel draws at a time (sched.hpp): 16 results are about one variable-base unit's work
#ifndef FB_CHUNK_UNITS
#define FB_CHUNK_UNITS 16
#endif
// occupancy target of the wide fixed-base kernel (3 = 168 VGPRs: 13.0-13.3 ms per 2^24 on P-256 against 12.5-12.6 at 4, fixedbase.hpp)
#ifndef FB_WIDE_WAVES
#define FB_WIDE_WAVES 4
#endif

// occupancy target (waves per SIMD) of the constant-time fixed-base kernel fb::mul_ct_kernel.  With the Jacobian addition (fixedbase_ct.hpp)
// the live set fits 128 VGPRs on the 8-word curves (k256: 10 spilled) and 168 on P-384 (15 spilled); signing per 2^20 at these against the
// round-2 targets 3 / 4 / 2: k256 4.66 vs 4.72 ms, p384 16.4 vs 17.1 ms (profiles/r03_ab_measurements.txt)
#ifndef FBCT_WAVES
#define FBCT_WAVES(C) (C::NW > 8 ? 3 : 4)
#endif

namespace ecgpu {

template <class C>
struct CurveOps {
  static int field_op(ecgpu_ctx* c, int op, const u32* a, const u32* b, u32* o, size_t n) {
    const unsigned g = ecgpu_grid_for(c, n, 8);
    switch (op) {
#define FOP(OPC) case OPC: hipLaunchKernelGGL((field_op_kernel<C, OPC>), dim3(g), dim3(256), 0, c->stream, a, b, o, n); break;
      FOP(FE_MUL) FOP(FE_SQR) FOP(FE_ADD) FOP(FE_SUB) FOP(FE_NEG) FOP(FE_INV) FOP(FE_SQRT)
#undef FOP
      default: return ecgpu_set_err(c, ECGPU_ERR_ARG, "unknown field op %d", op);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int point_op(ecgpu_ctx* c, int op, const u32* p, const u32* q, u32* o, size_t n) {
    const unsigned g = ecgpu_grid_for(c, n, 8);
    switch (op) {
      case PT_ADD: hipLaunchKernelGGL((point_op_kernel<C, PT_ADD>), dim3(g), dim3(256), 0, c->stream, p, q, o, n); break;
      case PT_ADD_MIXED: hipLaunchKernelGGL((point_op_kernel<C, PT_ADD_MIXED>), dim3(g), dim3(256), 0, c->stream, p, q, o, n); break;
      case PT_DOUBLE: hipLaunchKernelGGL((point_op_kernel<C, PT_DOUBLE>), dim3(g), dim3(256), 0, c->stream, p, q, o, n); break;
      default: return ecgpu_set_err(c, ECGPU_ERR_ARG, "unknown point op %d", op);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int normalize(ecgpu_ctx* c, const u32* p, u32* out_xy, uint8_t* out_inf, size_t n) {
    hipLaunchKernelGGL((normalize_kernel<C, 16>), dim3(ecgpu_grid_for((const ecgpu_ctx*)c, (n + 15) / 16, 8)), dim3(256), 0, c->stream, p, out_xy, out_inf, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int ensure_gen_table(ecgpu_ctx* c) {
    if (c->table[ECGPU_TAB_GEN][C::ID]) return 0;
    void* t = nullptr;
    HIPCHK(c, hipMalloc(&t, sizeof(typename C::Pt) * C::GEN_TABLE_PTS));
    hipLaunchKernelGGL((gen_table_kernel<C>), dim3(1), dim3(64), 0, c->stream, (typename C::Pt*)t);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));     // later calls may run on another stream (ecgpu_set_stream)
    c->table[ECGPU_TAB_GEN][C::ID] = t;
    return 0;
  }
  // fixed-base table T[j][d-1] = d 2^(8j) G (fixedbase.hpp), built once per context
  static constexpr int FB_NOMEM = 100;          // internal: a table did not fit, the caller steps down a width
  static void fb_account(ecgpu_ctx* c, size_t bytes, int window) {
    c->fb_bytes[C::ID] += bytes;
    if (window > c->fb_widest[C::ID]) c->fb_widest[C::ID] = window;
  }
  static int ensure_fb_table(ecgpu_ctx* c) {
    if (c->table[ECGPU_TAB_FB8][C::ID]) return 0;
    const int total = fb::nwin<C>() * fb::ENTRIES;
    struct Tmp {                       // released on every exit path
      void* p = nullptr;
      ~Tmp() { if (p) (void)hipFree(p); }
    } ttmp, ttab;
    HIPCHK(c, hipMalloc(&ttmp.p, sizeof(Jac<C>) * total));
    HIPCHK(c, hipMalloc(&ttab.p, sizeof(AffEntry<C>) * total));
    void *tmp = ttmp.p, *tab = ttab.p;
    hipLaunchKernelGGL((fb::table_jac_kernel<C>), dim3((fb::nwin<C>() + 63) / 64), dim3(64), 0, c->stream, (Jac<C>*)tmp);
    hipLaunchKernelGGL((fb::table_affine_kernel<C>), dim3((total + 255) / 256), dim3(256), 0, c->stream, (const Jac<C>*)tmp, (AffEntry<C>*)tab, total);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->table[ECGPU_TAB_FB8][C::ID] = tab;
    ttab.p = nullptr;                  // owned by the context from here on
    fb_account(c, sizeof(AffEntry<C>) * total, fb::W);
    return 0;
  }
  // wide tables TW[j][d-1] = d 2^(WB j) G, 2^(WB-1) entries per window, built by multiplying the scalars d 2^(WB j)
  // with the 8-bit-window kernel (WB <= 20) or the 20-bit-window kernel (WB > 20); used for large batches, where the
  // build cost (one pass over 0.56 M points for WB = 16, 6.8 M for WB = 20, 92 M for WB = 24, 336 M for WB = 26) is
  // amortised.  The 288 GB of HBM are what makes the last two possible: every window bit less is one mixed addition of
  // twelve saved per result, paid for with table bytes that a lane reads one 64-byte entry at a time.
  template <int WB>
  static int ensure_fb_wide_table(ecgpu_ctx* c, void** slot) {
    if (*slot) return 0;
    int rc = ensure_fb_table(c);
    if (rc) return rc;
    if constexpr (WB > 20) {
      if ((rc = ensure_fb_wide_table<20>(c, &c->table[ECGPU_TAB_FB20][C::ID]))) return rc;       // FB_NOMEM passes through
    }
    const size_t total = (size_t)fb::nwin_wide<C, WB>() * fb::wide_entries<WB>();
    const size_t chunk = total < ((size_t)1 << 24) ? total : ((size_t)1 << 24);     // entries per pass: at most 1.5 GB (2.3 GB for p384) of scratch
    struct Tmp {                       // released on every exit path
      void* p = nullptr;
      ~Tmp() { if (p) (void)hipFree(p); }
    } tks, txy, ttab;
    // a table that does not fit - the context's budget or the device's memory - is not an error: the caller falls back to
    // the next narrower width
    // (the budget is about the OPTIONAL wide tables: the 5-bit table of the constant-time kernel behind signing and key generation is
    // 53-80 KB and mandatory, like the 8-bit base table - neither is ever refused on the budget's account, though both count towards it)
    if (WB != fb::CT_WB && c->opt[ECGPU_OPT_FB_MEMORY_BUDGET] > 0 &&
        c->fb_bytes[C::ID] + total * sizeof(AffEntry<C>) > (size_t)c->opt[ECGPU_OPT_FB_MEMORY_BUDGET])
      return FB_NOMEM;
    {
      hipError_t e = hipMalloc(&tks.p, chunk * C::NB);
      if (e == hipSuccess) e = hipMalloc(&txy.p, chunk * 2 * C::NB);
      if (e == hipSuccess) e = hipMalloc(&ttab.p, total * sizeof(AffEntry<C>));
      if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();         // not sticky: the next launch check must not report it
        return FB_NOMEM;
      }
      if (e != hipSuccess) return ecgpu_set_err(c, ECGPU_ERR_RUNTIME, "generator table (%d-bit windows): %s", WB, hipGetErrorString(e));
    }
    void *ks = tks.p, *xy = txy.p;
    AffEntry<C>* tab = (AffEntry<C>*)ttab.p;
    for (size_t e0 = 0; e0 < total; e0 += chunk) {
      const size_t cnt = total - e0 < chunk ? total - e0 : chunk;
      hipLaunchKernelGGL((fb::table_scalars_kernel<C, WB>), dim3(ecgpu_grid_for(c, cnt, 8)), dim3(256), 0, c->stream, (u32*)ks, e0, cnt);
      if constexpr (WB > 20)
        hipLaunchKernelGGL((fb::mul_wide_kernel<C, 20, FB_BATCH, 4>), dim3(ecgpu_grid_for(c, cnt, 4)), dim3(256), 0, c->stream, (const u32*)ks,
                           (const AffEntry<C>*)c->table[ECGPU_TAB_FB20][C::ID], (u32*)xy, FMT_AFFINE, (uint8_t*)nullptr, cnt, WaveSched{nullptr, 0, 0, 0, 0});
      else
        hipLaunchKernelGGL((fb::mul_kernel<C, 16, 4>), dim3(ecgpu_grid_for(c, cnt, 4)), dim3(256), 0, c->stream, (const u32*)ks,
                           (const AffEntry<C>*)c->table[ECGPU_TAB_FB8][C::ID], (u32*)xy, FMT_AFFINE, (uint8_t*)nullptr, cnt);
      hipLaunchKernelGGL((fb::table_from_bytes_kernel<C>), dim3(ecgpu_grid_for(c, cnt, 8)), dim3(256), 0, c->stream, (const u32*)xy, tab + e0, cnt);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *slot = tab;
    ttab.p = nullptr;                  // the context owns the table now; the two scratch buffers go with this scope
    fb_account(c, total * sizeof(AffEntry<C>), WB);
    return 0;
  }
  template <int WB>
  static int mul_gen_wide(ecgpu_ctx* c, void** slot, const u32* sc, u32* out, int out_fmt, uint8_t* out_inf, size_t n) {
    int rc = ensure_fb_wide_table<WB>(c, slot);
    if (rc) return rc;
    return mul_wide_table<WB>(c, *slot, sc, out, out_fmt, out_inf, n);
  }
  // the wide kernel on any table of its layout: the generator's, or a shared point's (sharedbase.hpp)
  template <int WB>
  static int mul_wide_table(ecgpu_ctx* c, const void* table, const u32* sc, u32* out, int out_fmt, uint8_t* out_inf, size_t n) {
    unsigned long long* ctr = ecgpu_sched_counter(c);
    if (!ctr) return ECGPU_ERR_RUNTIME;
    // a chunk of 0 results never advances the work counter (the kernel hangs); one above the batch overruns the result buffer before its flush test
    static_assert(FB_CHUNK_UNITS >= 1 && FB_CHUNK_UNITS <= (FB_BATCH), "FB_CHUNK_UNITS must lie in 1 .. FB_BATCH");
    const unsigned grid = ecgpu_grid_for(c, n, FB_WIDE_WAVES);
    hipLaunchKernelGGL((fb::mul_wide_kernel<C, WB, FB_BATCH, FB_WIDE_WAVES>), dim3(grid), dim3(256), 0, c->stream, sc,
                       (const AffEntry<C>*)table, out, out_fmt, out_inf, n, WaveSched{ctr, (unsigned long long)n, grid * 4u, (unsigned)FB_CHUNK_UNITS, 1u});
    HIPCHK(c, hipGetLastError());
    return 1;
  }
  static int mul_gen_fast(ecgpu_ctx* c, const u32* sc, u32* out, int out_fmt, uint8_t* out_inf, size_t n) {
    // ECGPU_OPT_FB_WINDOW pins one table width (measurements, small-memory processes); ECGPU_OPT_FB_MAX_WINDOW caps what
    // the size rule may pick (default 26: 21.5 GB per 256-bit curve)
    const int forced = (int)c->opt[ECGPU_OPT_FB_WINDOW];
    // (P-384 stops at 24 bits: its 26-bit table would be 48 GB and measured 45.2 ms against 46.4 ms per 2^24 results)
    int wb = (n >= ((size_t)1 << 24) && C::NW <= 8) ? 26 : n >= ((size_t)1 << 23) ? 24 : n >= ((size_t)1 << 21) ? 20 : n >= ((size_t)1 << 18) ? 16 : 8;
    if (forced) wb = forced;
    // A table that cannot be allocated is not an error: step down to the next narrower one and remember the width that
    // fitted as this context's cap, so that later calls do not try (and fail) a 21 GB allocation each time.
    for (;;) {
      const int cap = (int)c->opt[ECGPU_OPT_FB_MAX_WINDOW];
      if (wb > cap) wb = cap;
      int rc;
      if (wb >= 26) rc = mul_gen_wide<26>(c, &c->table[ECGPU_TAB_FB26][C::ID], sc, out, out_fmt, out_inf, n);
      else if (wb >= 24) rc = mul_gen_wide<24>(c, &c->table[ECGPU_TAB_FB24][C::ID], sc, out, out_fmt, out_inf, n);
      else if (wb >= 20) rc = mul_gen_wide<20>(c, &c->table[ECGPU_TAB_FB20][C::ID], sc, out, out_fmt, out_inf, n);
      else if (wb >= 16) rc = mul_gen_wide<16>(c, &c->table[ECGPU_TAB_FB16][C::ID], sc, out, out_fmt, out_inf, n);
      else break;
      if (rc != FB_NOMEM) return rc;
      wb = wb >= 26 ? 24 : wb >= 24 ? 20 : wb >= 20 ? 16 : 8;
      c->opt[ECGPU_OPT_FB_MAX_WINDOW] = wb;
    }
    int rc = ensure_fb_table(c);
    if (rc) return rc;
    hipLaunchKernelGGL((fb::mul_kernel<C, 16, 4>), dim3(ecgpu_grid_for(c, n, 4)), dim3(256), 0, c->stream, sc,
                       (const AffEntry<C>*)c->table[ECGPU_TAB_FB8][C::ID], out, out_fmt, out_inf, n);
    HIPCHK(c, hipGetLastError());
    return 1;
  }
  // k G for secret scalars: constant-time fixed-base kernel (fixedbase.hpp), one inversion per 8 results
  static int mul_gen_ct(ecgpu_ctx* c, const u32* sc, u32* out, int out_fmt, uint8_t* out_inf, size_t n) {
    int rc = ensure_fb_wide_table<fb::CT_WB>(c, &c->table[ECGPU_TAB_FBCT][C::ID]);
    if (rc == FB_NOMEM) return ecgpu_set_err(c, ECGPU_ERR_RUNTIME, "hipMalloc failed (out of device memory) for the 5-bit generator table of the constant-time kernel");
    if (rc) return rc;
    return mul_ct_table(c, c->table[ECGPU_TAB_FBCT][C::ID], sc, out, out_fmt, out_inf, n);
  }
  // the constant-time kernel on any 5-bit table: the generator's, or a shared point's (fixedbase_ct.hpp: the argument needs the base's order only)
  static int mul_ct_table(ecgpu_ctx* c, const void* table, const u32* sc, u32* out, int out_fmt, uint8_t* out_inf, size_t n) {
    if constexpr (C::ID == 0) {          // secp256k1: the kernel lives in the branch-free translation unit (ops_k256_ct.hip)
      return ecgpuint_k256_mul_gen_ct(c, sc, table, out, out_fmt, out_inf, n);
    } else {
      constexpr int WAVES = FBCT_WAVES(C);
      hipLaunchKernelGGL((fb::mul_ct_kernel<C, 8, WAVES>), dim3(ecgpu_grid_oversubscribed(c, n, WAVES, 8, FBCT_GRID_MULT)), dim3(256), 0, c->stream, sc, (const AffEntry<C>*)table, out,
                         out_fmt, out_inf, n);
      HIPCHK(c, hipGetLastError());
      return 0;
    }
  }
  // ---- shared points (sharedbase.hpp): the launchers behind ECGPU_SHARED_POINTS; which table a call uses is the API layer's business
  static_assert(fb::SHARED_MAX_TERMS == ECGPU_SHARED_MAX_TERMS, "the API layer plans for as many tables as one launch reads");
  static size_t shared_table_bytes(int wb) {
    switch (wb) {
      case fb::CT_WB: return sizeof(AffEntry<C>) * (size_t)fb::nwin_wide<C, fb::CT_WB>() * fb::wide_entries<fb::CT_WB>();
      case 8: return sizeof(AffEntry<C>) * (size_t)fb::nwin_wide<C, 8>() * fb::wide_entries<8>();
      case 16: return sizeof(AffEntry<C>) * (size_t)fb::nwin_wide<C, 16>() * fb::wide_entries<16>();
      case 20: return sizeof(AffEntry<C>) * (size_t)fb::nwin_wide<C, 20>() * fb::wide_entries<20>();
      default: return 0;
    }
  }
  template <int WB>
  static int shared_build_w(ecgpu_ctx* c, const u32* xy, void* bases, void* table) {
    constexpr int NWIN = fb::nwin_wide<C, WB>();
    const size_t runs = (size_t)NWIN * (fb::wide_entries<WB>() / fb::SHARED_RUN);
    hipLaunchKernelGGL((fb::shared_bases_kernel<C, WB>), dim3((NWIN + 63) / 64), dim3(64), 0, c->stream, xy, (AffEntry<C>*)bases);
    hipLaunchKernelGGL((fb::shared_runs_kernel<C, WB>), dim3(ecgpu_grid_for(c, runs, 8)), dim3(256), 0, c->stream, (const AffEntry<C>*)bases,
                       (AffEntry<C>*)table, runs);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int shared_build(ecgpu_ctx* c, const u32* xy, int wb, void* bases, void* table) {
    switch (wb) {
      case fb::CT_WB: return shared_build_w<fb::CT_WB>(c, xy, bases, table);
      case 8: return shared_build_w<8>(c, xy, bases, table);
      case 16: return shared_build_w<16>(c, xy, bases, table);
      case 20: return shared_build_w<20>(c, xy, bases, table);
      default: return ecgpu_set_err(c, ECGPU_ERR_ARG, "shared points: no table of %d-bit windows", wb);
    }
  }
  template <int WB>
  static int shared_lincomb_w(ecgpu_ctx* c, const u32* sc, const void* const* tables, size_t terms, u32* out, int out_fmt, uint8_t* out_inf, size_t n) {
    fb::SharedTabs<C> tabs;
    for (int t = 0; t < fb::SHARED_MAX_TERMS; t++) tabs.t[t] = t < (int)terms ? (const AffEntry<C>*)tables[t] : nullptr;
    tabs.terms = (int)terms;
    unsigned long long* ctr = ecgpu_sched_counter(c);
    if (!ctr) return ECGPU_ERR_RUNTIME;
    const unsigned grid = ecgpu_grid_for(c, n, FB_WIDE_WAVES);
    hipLaunchKernelGGL((fb::mul_shared_kernel<C, WB, FB_BATCH, FB_WIDE_WAVES>), dim3(grid), dim3(256), 0, c->stream, sc, tabs, out, out_fmt, out_inf, n,
                       WaveSched{ctr, (unsigned long long)n, grid * 4u, (unsigned)FB_CHUNK_UNITS, 1u});
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int shared_lincomb(ecgpu_ctx* c, const u32* sc, const void* const* tables, int wb, size_t terms, u32* out, int out_fmt, uint8_t* out_inf, size_t n,
                            unsigned flags) {
    if (terms < 1 || terms > (size_t)fb::SHARED_MAX_TERMS) return ecgpu_set_err(c, ECGPU_ERR_ARG, "shared points: 1 .. %d tables per launch", fb::SHARED_MAX_TERMS);
    if (flags & ECGPU_SECRET_SCALARS) {
      if (terms != 1 || wb != fb::CT_WB || !tables[0]) return ecgpu_set_err(c, ECGPU_ERR_ARG, "shared points: secret scalars take one 5-bit table");
      return mul_ct_table(c, tables[0], sc, out, out_fmt, out_inf, n);
    }
    // one table: the generator's kernels, unchanged (a positive return is their "launched")
    if (terms == 1 && tables[0]) {
      if (wb == 20) { int rc = mul_wide_table<20>(c, tables[0], sc, out, out_fmt, out_inf, n); return rc < 0 ? rc : 0; }
      if (wb == 16) { int rc = mul_wide_table<16>(c, tables[0], sc, out, out_fmt, out_inf, n); return rc < 0 ? rc : 0; }
      if (wb == 8) {
        hipLaunchKernelGGL((fb::mul_kernel<C, 16, 4>), dim3(ecgpu_grid_for(c, n, 4)), dim3(256), 0, c->stream, sc, (const AffEntry<C>*)tables[0], out, out_fmt, out_inf, n);
        HIPCHK(c, hipGetLastError());
        return 0;
      }
    }
    switch (wb) {
      case 8: return shared_lincomb_w<8>(c, sc, tables, terms, out, out_fmt, out_inf, n);
      case 16: return shared_lincomb_w<16>(c, sc, tables, terms, out, out_fmt, out_inf, n);
      case 20: return shared_lincomb_w<20>(c, sc, tables, terms, out, out_fmt, out_inf, n);
      default: return ecgpu_set_err(c, ECGPU_ERR_ARG, "shared points: no kernel for %d-bit windows", wb);
    }
  }
  static int broadcast_points(ecgpu_ctx* c, const u32* xy, size_t terms, u32* dst, size_t n) {
    hipLaunchKernelGGL((fb::broadcast_points_kernel<C>), dim3(ecgpu_grid_for(c, n * terms * 2 * C::NW, 8)), dim3(256), 0, c->stream, xy, terms * 2 * C::NW, dst, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  // curve-specific throughput kernels hook in here (specialised in ops_*.hip); returns 1 if it launched
  static int lincomb_fast(ecgpu_ctx* c, const u32* sc, const u32* pts, int pt_fmt, size_t terms, u32* out, int out_fmt,
                          uint8_t* out_inf, size_t n);
  // constant-time variable base for secret scalars (varbase_ct.hpp; specialised in ops_*.hip); returns 1 if it launched
  static int mul_ct(ecgpu_ctx* c, const u32* sc, const u32* pts, int pt_fmt, u32* out, int out_fmt, uint8_t* out_inf, size_t n);
  static int lincomb(ecgpu_ctx* c, const u32* sc, const u32* pts, int pt_fmt, size_t terms, u32* out, int out_fmt, uint8_t* out_inf,
                     size_t n, unsigned flags) {
    if ((flags & ECGPU_SECRET_SCALARS) && !(flags & ECGPU_EXACT_REFERENCE)) {
      if (!pts && terms == 1) return mul_gen_ct(c, sc, out, out_fmt, out_inf, n);
      if (pts && terms == 1) {
        int rc = mul_ct(c, sc, pts, pt_fmt, out, out_fmt, out_inf, n);
        if (rc < 0) return rc;
        if (rc == 1) return 0;
      }
      flags |= ECGPU_EXACT_REFERENCE;              // no dedicated kernel: the reference schedule is constant-time as well
    }
    if (!(flags & ECGPU_EXACT_REFERENCE)) {
      int rc = lincomb_fast(c, sc, pts, pt_fmt, terms, out, out_fmt, out_inf, n);
      if (rc < 0) return rc;
      if (rc == 1) return 0;
    }
    // (the reference-schedule kernels walk their units one at a time with a grid stride: four times the workgroups the chip holds, so that the hardware
    // hands the waiting ones out as the favoured waves of a SIMD leave - sched.hpp)
    const unsigned g = ecgpu_grid_for(c, n, 4 * ECGPU_REF_GRID_MULT);
    if (!pts && terms != 1) return ecgpu_set_err(c, ECGPU_ERR_ARG, "generator multiplication takes one term");
    if (terms > 2 && terms <= 1024 && !(flags & ECGPU_EXACT_REFERENCE)) {
      if (c->opt[ECGPU_OPT_LINCOMB_TERM_BY_TERM]) {
        hipLaunchKernelGGL((lincomb_sum_kernel<C>), dim3(g), dim3(256), 0, c->stream, sc, pts, pt_fmt, (int)terms, out, out_fmt, out_inf, n);
        HIPCHK(c, hipGetLastError());
        return 0;
      }
      return lincomb_straus(c, sc, pts, pt_fmt, terms, out, out_fmt, out_inf, n);
    }
    if (terms > 1024 || (terms > 2 && C::ID != 0))
      return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED,
                           "lincomb_batch: at most 1024 terms per combination (use ecgpu_msm for one large sum); ECGPU_EXACT_REFERENCE with more than 2 terms "
                           "exists for secp256k1 only (the primeorder curves have no in-tree lincomb over slices to be exact to)");
    // the reference schedules (exact X, Y, Z; constant-time table scans)
    if (!pts) {
      int rc = ensure_gen_table(c);
      if (rc) return rc;
    }
    if constexpr (C::ID == 0) {            // secp256k1: in the branch-free translation unit (ops_k256_ct.hip)
      return ecgpuint_k256_reference(c, sc, pts, pt_fmt, terms, c->table[ECGPU_TAB_GEN][C::ID], out, out_fmt, out_inf, n);
    } else {
      if (!pts) {
        hipLaunchKernelGGL((mul_gen_ref_kernel<C>), dim3(g), dim3(256), 0, c->stream, sc, (const typename C::Pt*)c->table[ECGPU_TAB_GEN][C::ID], out,
                           out_fmt, out_inf, n);
      } else if (terms == 1) {
        hipLaunchKernelGGL((lincomb_ref_kernel<C, 1>), dim3(g), dim3(256), 0, c->stream, sc, pts, pt_fmt, out, out_fmt, out_inf, n);
      } else {
        hipLaunchKernelGGL((lincomb_ref_kernel<C, 2>), dim3(g), dim3(256), 0, c->stream, sc, pts, pt_fmt, out, out_fmt, out_inf, n);
      }
      HIPCHK(c, hipGetLastError());
      return 0;
    }
  }
  // 3 .. 1024 terms per combination, throughput schedule (straus.hpp): groups of up to 16 terms share the doublings of one window
  // loop over per-term affine tables; a second small kernel adds the groups' partial sums and writes the outputs
  static int lincomb_straus(ecgpu_ctx* c, const u32* sc, const u32* pts, int pt_fmt, size_t terms, u32* out, int out_fmt, uint8_t* out_inf, size_t n) {
    // waves per SIMD: secp256k1 runs 3 (168 VGPRs: 22 spilled instead of 119 at 4; -3 .. -5 % at 3 .. 64 terms), P-256 measures equal and
    // P-384 was not timed at 3: both keep 4 (profiles/r04_ab_measurements.txt, set twelve)
    constexpr int WAVES = C::ID == 0 ? 3 : 4;
    int g, gpc;
    straus::plan(n, terms, resident_lanes(c, WAVES), &g, &gpc);
    const size_t items = n * (size_t)gpc, upp = (size_t)(straus::SLOTS / g);
    const unsigned grid = ecgpu_grid_for(c, (items + upp - 1) / upp, WAVES);
    int rc = ecgpu_reserve(c, c->tab_ws, (size_t)grid * 256 * sizeof(straus::LaneWs<C>));
    if (rc) return rc;
    u32* partial;
    if ((rc = ecgpu_carve(c, c->ecdsa_ws, [&](WsCarver& ws) { partial = ws.take<u32>(items * 3 * C::NW * sizeof(u32)); }))) return rc;
    unsigned long long* ctr = ecgpu_sched_counter(c);
    if (!ctr) return ECGPU_ERR_RUNTIME;
    hipLaunchKernelGGL((straus::lincomb_kernel<C, WAVES>), dim3(grid), dim3(256), 0, c->stream, sc, pts, pt_fmt, (int)terms, g, gpc, items,
                       (straus::LaneWs<C>*)c->tab_ws.p, partial, WaveSched{ctr, (unsigned long long)items, grid * 4u, (unsigned)upp, 0u});
    hipLaunchKernelGGL((straus::fold_kernel<C>), dim3(ecgpu_grid_for(c, (n + 15) / 16, 8)), dim3(256), 0, c->stream, (const u32*)partial, gpc, out, out_fmt, out_inf, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int msm(ecgpu_ctx* c, const u32* sc, const u32* pts, int pt_fmt, size_t n, u32* out, int out_fmt);
  // resident lanes at `waves` workgroups of 256 per CU (what ecgpu_grid_for caps a grid at)
  static size_t resident_lanes(const ecgpu_ctx* c, int waves) { return (size_t)c->num_cus * (size_t)waves * 256; }
  // units per whole pass of the variable-base kernels (specialised in ops_*.hip, where their sub-batch sizes are)
  static size_t pass_units_points(const ecgpu_ctx* c, size_t terms, unsigned flags);
  static size_t pass_units(const ecgpu_ctx* c, int has_points, size_t terms, unsigned flags) {
    if (has_points) return pass_units_points(c, terms, flags);
    if ((flags & ECGPU_SECRET_SCALARS) && !(flags & ECGPU_EXACT_REFERENCE)) return resident_lanes(c, FBCT_WAVES(C)) * 8;   // fb::mul_ct_kernel<C, 8, ..>
    if (flags & ECGPU_EXACT_REFERENCE) return resident_lanes(c, 4);
    return resident_lanes(c, 4) * (size_t)(FB_BATCH);                                                                    // fb::mul_wide_kernel<C, .., FB_BATCH, 4>
  }
  static int point_eq(ecgpu_ctx* c, const u32* p, const u32* q, uint8_t* eq, size_t n) {
    hipLaunchKernelGGL((point_eq_kernel<C>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, p, q, eq, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int validate_scalars(ecgpu_ctx* c, const u32* sc, uint8_t* ok, size_t n, size_t terms) {
    hipLaunchKernelGGL((validate_scalars_kernel<C>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, sc, ok, n, terms);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int validate_points(ecgpu_ctx* c, const u32* xy, uint8_t* ok, size_t n) {
    hipLaunchKernelGGL((validate_points_kernel<C>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, xy, ok, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int decompress(ecgpu_ctx* c, const u32* x, const uint8_t* odd, u32* out_xy, uint8_t* ok, size_t n) {
    hipLaunchKernelGGL((decompress_kernel<C>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, x, odd, out_xy, ok, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int synth_scalars(ecgpu_ctx* c, uint64_t seed, uint64_t first, u32* out, size_t n) {
    hipLaunchKernelGGL((synth_scalars_kernel<C>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, (u64)seed, (u64)first, out, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int synth_points(ecgpu_ctx* c, uint64_t seed, uint64_t first, u32* out, size_t n) {
    hipLaunchKernelGGL((synth_points_kernel<C>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, (u64)seed, (u64)first, out, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  // GroupEncoding::to_bytes / ToEncodedPoint of affine or projective points (projective input is batch-normalised first)
  static int sec1_to(ecgpu_ctx* c, const u32* pts, int pt_fmt, int uncompressed, uint8_t* out, size_t n) {
    const u32* xy = pts;
    const uint8_t* inf = nullptr;
    if (pt_fmt == FMT_PROJECTIVE) {
      u32* t;
      uint8_t* ti;
      int rc = ecgpu_carve(c, c->ecdsa_ws, [&](WsCarver& ws) { t = ws.take<u32>(n * 2 * C::NB); ti = ws.take<uint8_t>(n); });
      if (rc) return rc;
      if ((rc = normalize(c, pts, t, ti, n))) return rc;
      xy = t; inf = ti;
    }
    hipLaunchKernelGGL((sec1::to_bytes_kernel<C>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, xy, inf, out, n, uncompressed);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int to_bytes(ecgpu_ctx* c, const u32* pts, int pt_fmt, uint8_t* out, size_t n) { return sec1_to(c, pts, pt_fmt, 0, out, n); }
  static int sec1_encode(ecgpu_ctx* c, const u32* pts, int pt_fmt, int compress, uint8_t* out, size_t n) { return sec1_to(c, pts, pt_fmt, compress ? 0 : 1, out, n); }
  static int sec1_decode(ecgpu_ctx* c, const uint8_t* in, size_t record_bytes, u32* out_xy, uint8_t* ok, size_t n) {
    hipLaunchKernelGGL((sec1::from_bytes_kernel<C>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, in, out_xy, ok, n, (int)record_bytes);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int from_bytes(ecgpu_ctx* c, const uint8_t* in, u32* out_xy, uint8_t* ok, size_t n) { return sec1_decode(c, in, 1 + C::NB, out_xy, ok, n); }
  // ECDSA / BIP340 verification and key recovery (ecdsa_kernels.hpp, schnorr_kernels.hpp) share one shape: a prep kernel writes the
  // scalars u1, u2 (recovery and BIP340: a point `pt` as well), u1 G and u2 Q run on the throughput kernels above, a last kernel
  // compares or combines the two products a and b.  The intermediates live in the workspace in the order of these members.
  struct VerifyWs {
    u32 *u1, *u2, *pt, *a, *b;
    uint8_t *a_inf, *b_inf;
  };
  static void verify_layout(WsCarver& ws, size_t n, bool with_pt, VerifyWs& w) {
    w.u1 = ws.take<u32>(n * C::NB);
    w.u2 = ws.take<u32>(n * C::NB);
    w.pt = with_pt ? ws.take<u32>(n * 2 * C::NB) : nullptr;
    w.a = ws.take<u32>(n * 2 * C::NB);
    w.b = ws.take<u32>(n * 2 * C::NB);
    w.a_inf = ws.take<uint8_t>(n);
    w.b_inf = ws.take<uint8_t>(n);
  }
  static int verify_ws(ecgpu_ctx* c, size_t n, bool with_pt, VerifyWs& w) {
    return ecgpu_carve(c, c->ecdsa_ws, [&](WsCarver& ws) { verify_layout(ws, n, with_pt, w); });
  }
  // a = u1 G, b = u2 Q (after the prep kernel's launch check).  One term each: lincomb cannot reach lincomb_straus, which carves ecdsa_ws.
  static int verify_products(ecgpu_ctx* c, const VerifyWs& w, const u32* q, size_t n) {
    HIPCHK(c, hipGetLastError());
    int rc = lincomb(c, w.u1, nullptr, FMT_AFFINE, 1, w.a, FMT_AFFINE, w.a_inf, n, 0);
    if (rc) return rc;
    return lincomb(c, w.u2, q, FMT_AFFINE, 1, w.b, FMT_AFFINE, w.b_inf, n, 0);
  }
  static int ecdsa_verify(ecgpu_ctx* c, const u32* z, const u32* sig, const u32* q, uint8_t* ok, size_t n, unsigned flags) {
    VerifyWs w;
    int rc = verify_ws(c, n, false, w);
    if (rc) return rc;
    hipLaunchKernelGGL((ecdsa::verify_prep_kernel<C, 16>), dim3(ecgpu_grid_for(c, (n + 15) / 16, 4)), dim3(256), 0, c->stream, z, sig, q, w.u1, w.u2,
                       ok, n, flags);
    if ((rc = verify_products(c, w, q, n))) return rc;
    hipLaunchKernelGGL((ecdsa::verify_check_kernel<C>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, (const u32*)w.a,
                       (const uint8_t*)w.a_inf, (const u32*)w.b, (const uint8_t*)w.b_inf, sig, ok, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  // ecdsa_verify against ONE valid key Q: q_rep holds Q n times, so the prep kernel computes what it computes for a per-element
  // call; a = u1 G as there, b = u2 Q from Q's table
  static int ecdsa_verify_shared(ecgpu_ctx* c, const u32* z, const u32* sig, const u32* q_rep, const void* table, int wb, uint8_t* ok, size_t n,
                                 unsigned flags) {
    VerifyWs w;
    int rc = verify_ws(c, n, false, w);
    if (rc) return rc;
    hipLaunchKernelGGL((ecdsa::verify_prep_kernel<C, 16>), dim3(ecgpu_grid_for(c, (n + 15) / 16, 4)), dim3(256), 0, c->stream, z, sig, q_rep, w.u1, w.u2,
                       ok, n, flags);
    HIPCHK(c, hipGetLastError());
    if ((rc = lincomb(c, w.u1, nullptr, FMT_AFFINE, 1, w.a, FMT_AFFINE, w.a_inf, n, 0))) return rc;
    if ((rc = shared_lincomb(c, w.u2, &table, wb, 1, w.b, FMT_AFFINE, w.b_inf, n, 0))) return rc;
    hipLaunchKernelGGL((ecdsa::verify_check_kernel<C>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, (const u32*)w.a,
                       (const uint8_t*)w.a_inf, (const u32*)w.b, (const uint8_t*)w.b_inf, sig, ok, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int h2c_map(ecgpu_ctx* c, const u32* u, int count, u32* out_xy, uint8_t* out_inf, size_t n) {
    hipLaunchKernelGGL((h2c::map_kernel<C>), dim3(ecgpu_grid_for(c, n, 4)), dim3(256), 0, c->stream, u, count, out_xy, out_inf, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int ecdsa_recover(ecgpu_ctx* c, const u32* z, const u32* sig, const uint8_t* recid, u32* out_xy, uint8_t* ok, size_t n, unsigned flags) {
    VerifyWs w;
    int rc = verify_ws(c, n, true, w);
    if (rc) return rc;
    hipLaunchKernelGGL((ecdsa::recover_prep_kernel<C, 16>), dim3(ecgpu_grid_for(c, (n + 15) / 16, 4)), dim3(256), 0, c->stream, z, sig, recid, w.pt, w.u1,
                       w.u2, ok, n, flags);
    if ((rc = verify_products(c, w, w.pt, n))) return rc;
    hipLaunchKernelGGL((ecdsa::recover_finish_kernel<C, 16>), dim3(ecgpu_grid_for(c, (n + 15) / 16, 8)), dim3(256), 0, c->stream, (const u32*)w.a,
                       (const uint8_t*)w.a_inf, (const u32*)w.b, (const uint8_t*)w.b_inf, out_xy, ok, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  // BIP340 verification (schnorr_kernels.hpp), secp256k1 only.  The body runs on the caller's workspace layout (with_pt).
  static int schnorr_verify_body(ecgpu_ctx* c, const VerifyWs& w, const u32* px, const u32* sig, const u32* e, uint8_t* ok, size_t n) {
    if constexpr (C::ID != 0) {
      return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "ecgpu_schnorr_verify_batch: BIP340 is defined over secp256k1 only");
    } else {
      hipLaunchKernelGGL((schnorr::verify_prep_kernel<0>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, px, sig, e, w.pt, w.u1, w.u2, ok, n);
      int rc = verify_products(c, w, w.pt, n);
      if (rc) return rc;
      hipLaunchKernelGGL((schnorr::verify_check_kernel<16>), dim3(ecgpu_grid_for(c, (n + 15) / 16, 8)), dim3(256), 0, c->stream, (const u32*)w.a,
                         (const uint8_t*)w.a_inf, (const u32*)w.b, (const uint8_t*)w.b_inf, sig, ok, n);
      HIPCHK(c, hipGetLastError());
      return 0;
    }
  }
  static int schnorr_verify(ecgpu_ctx* c, const u32* px, const u32* sig, const u32* e, uint8_t* ok, size_t n) {
    if constexpr (C::ID != 0) {
      return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "ecgpu_schnorr_verify_batch: BIP340 is defined over secp256k1 only");
    } else {
      VerifyWs w;
      int rc = verify_ws(c, n, true, w);
      if (rc) return rc;
      return schnorr_verify_body(c, w, px, sig, e, ok, n);
    }
  }
  // BIP340 batch verification (schnorr_batch_kernels.hpp): one equation over the n signatures of this call, elements first_index ..
  // of the caller's batch.  prep (terms 0 .. 2n - 1, dec, the partial sums of a_i s_i) -> finish (term 2n) -> msm over 2n + 1 terms
  // -> the point and the count of left-out elements come to the host: the equation holds iff Z = 0.  Then ok = dec; otherwise
  // the per-signature body runs over the whole call, unless ECGPU_BATCH_VERDICT_ONLY asks for zeros.  ok may be NULL with that flag.
  // ONE carve of ecdsa_ws: the equation's buffers and the fallback's VerifyWs lie over the same bytes, the fallback starting when the
  // equation's buffers are dead.  msm carves msm_ws only - its small-sum path too: msm_run's carve (msm_kernels.hpp) names msm_ws, and its
  // `mul` is lincomb on ONE term (ops_*.hip), which reaches lincomb_fast / the reference kernels (tab_ws), never lincomb_straus.
  static int schnorr_batch_verify(ecgpu_ctx* c, const u32* px, const u32* sig, const u32* e, uint8_t* ok, size_t n, uint64_t first_index,
                                  const uint8_t* seed32, unsigned flags, int* verdict) {
    if constexpr (C::ID != 0) {
      return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "ecgpu_schnorr_batch_verify: BIP340 is defined over secp256k1 only");
    } else {
      namespace sb = schnorr_batch;
      if (n >= ((size_t)1 << 31)) return ecgpu_set_err(c, ECGPU_ERR_ARG, "ecgpu_schnorr_batch_verify: at most 2^31 - 1 signatures per equation");
      const bool verdict_only = (flags & ECGPU_BATCH_VERDICT_ONLY) != 0;
      const size_t terms = 2 * n + 1;
      const unsigned grid = ecgpu_grid_for(c, n, 8);
      u32 *sc, *pts, *partial, *res;
      uint8_t* dec;
      VerifyWs w;
      int rc = ecgpu_carve(c, c->ecdsa_ws, [&](WsCarver& ws) {
        sc = ws.take<u32>(terms * C::NB);                    // first: ecgpu_debug_workspace 1 shows the scalars at offset 0
        pts = ws.take<u32>(terms * 2 * C::NB);
        partial = ws.take<u32>((size_t)grid * sb::PARTIAL_WORDS * sizeof(u32));
        res = ws.take<u32>(32 * sizeof(u32));                // 24 words of X : Y : Z, then the count of left-out elements
        dec = ws.take<uint8_t>(n);
        const size_t equation_bytes = ws.total;
        ws.total = 0;
        if (!verdict_only) verify_layout(ws, n, true, w);
        if (ws.total < equation_bytes) ws.total = equation_bytes;
      });
      if (rc) return rc;
      if (ok) dec = ok;                                      // ok = dec where the equation holds; overwritten where it does not
      sb::Seed seed;
      for (int i = 0; i < 8; i++)
        seed.w[i] = (u32)seed32[4 * i] << 24 | (u32)seed32[4 * i + 1] << 16 | (u32)seed32[4 * i + 2] << 8 | (u32)seed32[4 * i + 3];
      hipLaunchKernelGGL((sb::prep_kernel<0>), dim3(grid), dim3(256), 0, c->stream, px, sig, e, seed, (u64)first_index, sc, pts, dec, partial, n);
      hipLaunchKernelGGL((sb::finish_kernel<0>), dim3(1), dim3(64), 0, c->stream, (const u32*)partial, (int)grid, sc + 2 * n * C::NW,
                         pts + 2 * n * 2 * C::NW, res + 24);
      HIPCHK(c, hipGetLastError());
      if ((rc = msm(c, sc, pts, FMT_AFFINE, terms, res, FMT_PROJECTIVE))) return rc;
      u32 host_res[25];
      HIPCHK(c, hipMemcpyAsync(host_res, res, sizeof(host_res), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      u32 z = 0;
      for (int i = 16; i < 24; i++) z |= host_res[i];
      const bool holds = z == 0;
      *verdict = (holds && host_res[24] == 0) ? 1 : 0;
      if (holds) return 0;
      if (verdict_only) {
        if (ok) HIPCHK(c, hipMemsetAsync(ok, 0, n, c->stream));
        return 0;
      }
      return schnorr_verify_body(c, w, px, sig, e, ok, n);
    }
  }
  // ECDH (ecdh_kernels.hpp): input checks, the secret-scalar multiplication (constant-time kernel where the curve has
  // one, the reference schedule otherwise), x of the product
  static int ecdh(ecgpu_ctx* c, const u32* d, const u32* q, u32* shared_x, uint8_t* ok, size_t n) {
    u32 *prod, *q_sane;
    int rc = ecgpu_carve(c, c->ecdsa_ws, [&](WsCarver& ws) { prod = ws.take<u32>(n * 2 * C::NB); q_sane = ws.take<u32>(n * 2 * C::NB); });
    if (rc) return rc;
    // the products are secrets of the same rank as the shared values handed back: they do not stay in the workspace, whichever way
    // this function is left (the constant-time kernels clear what they park in the table workspace themselves)
    StreamWipe prod_wipe{c, prod, n * 2 * C::NB};
    hipLaunchKernelGGL((ecdh::prep_kernel<C>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, d, q, q_sane, ok, n);
    HIPCHK(c, hipGetLastError());
    if ((rc = lincomb(c, d, q_sane, FMT_AFFINE, 1, prod, FMT_AFFINE, nullptr, n, (unsigned)ECGPU_SECRET_SCALARS))) return rc;
    hipLaunchKernelGGL((ecdh::finish_kernel<C>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, (const u32*)prod, (const uint8_t*)ok, shared_x, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  // R = k G into r_xy / r_inf (the caller's, out of its workspace layout), then the finish kernel
  static int ecdsa_sign_body(ecgpu_ctx* c, const u32* d, const u32* k, const u32* z, u32* r_xy, uint8_t* r_inf, u32* sig, uint8_t* recid, uint8_t* ok,
                             size_t n, unsigned flags) {
    int rc;
    // The nonce is secret: k G runs on the constant-time fixed-base kernel (every table entry read, one masked addition per window,
    // no digit-dependent branch or address) - or, with ECGPU_EXACT_REFERENCE, on the reference's own mul_by_generator
    // schedule, which is constant-time as well - unless the caller declares the scalars public.
    if (flags & ECGPU_PUBLIC_SCALARS) rc = lincomb(c, k, nullptr, FMT_AFFINE, 1, r_xy, FMT_AFFINE, r_inf, n, 0u);
    else if (flags & ECGPU_EXACT_REFERENCE) rc = lincomb(c, k, nullptr, FMT_AFFINE, 1, r_xy, FMT_AFFINE, r_inf, n, (unsigned)ECGPU_EXACT_REFERENCE);
    else rc = mul_gen_ct(c, k, r_xy, FMT_AFFINE, r_inf, n);
    if (rc) return rc;
    hipLaunchKernelGGL((ecdsa::sign_finish_kernel<C, 16>), dim3(ecgpu_grid_for(c, (n + 15) / 16, 4)), dim3(256), 0, c->stream, d, k, z,
                       (const u32*)r_xy, (const uint8_t*)r_inf, sig, recid, ok, n, flags);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int ecdsa_sign(ecgpu_ctx* c, const u32* d, const u32* k, const u32* z, u32* sig, uint8_t* recid, uint8_t* ok, size_t n,
                        unsigned flags) {
    u32* r_xy;
    uint8_t* r_inf;
    int rc = ecgpu_carve(c, c->ecdsa_ws, [&](WsCarver& ws) { r_xy = ws.take<u32>(n * 2 * C::NB); r_inf = ws.take<uint8_t>(n); });
    if (rc) return rc;
    return ecdsa_sign_body(c, d, k, z, r_xy, r_inf, sig, recid, ok, n, flags);
  }
  // Deterministic signing (signing_kernels.hpp).  The derived nonces pass through the intermediate workspace and are secrets of the
  // key's rank: they are cleared on the stream whichever way the launcher is left (the fixed-base kernels keep nothing of a scalar).
  static int rfc6979_nonce(ecgpu_ctx* c, const u32* d, const u32* z, const u32* extra, u32* k, size_t n) {
    const unsigned g = ecgpu_grid_for(c, n, 8);
    if (extra) hipLaunchKernelGGL((sign::rfc6979_nonce_kernel<C, true>), dim3(g), dim3(256), 0, c->stream, d, z, extra, k, n);
    else hipLaunchKernelGGL((sign::rfc6979_nonce_kernel<C, false>), dim3(g), dim3(256), 0, c->stream, d, z, extra, k, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int ecdsa_sign_prehash(ecgpu_ctx* c, const u32* d, const u32* z, const u32* extra, u32* sig, uint8_t* recid, uint8_t* ok, size_t n, unsigned flags) {
    u32 *r_xy, *k;
    uint8_t* r_inf;
    int rc = ecgpu_carve(c, c->ecdsa_ws, [&](WsCarver& ws) {
      r_xy = ws.take<u32>(n * 2 * C::NB);
      r_inf = ws.take<uint8_t>(n);
      k = ws.take<u32>(n * C::NB);
    });
    if (rc) return rc;
    StreamWipe wipe{c, k, n * C::NB};
    if ((rc = rfc6979_nonce(c, d, z, extra, k, n))) return rc;
    return ecdsa_sign_body(c, d, k, z, r_xy, r_inf, sig, recid, ok, n, flags);
  }
  // BIP340 (secp256k1 only): P = d G, the nonce kernel, R = k G, the finish kernel
  static int schnorr_sign_prehash(ecgpu_ctx* c, const u32* d, const u32* m, const u32* aux, u32* sig, u32* pubkeys_x, uint8_t* ok, size_t n) {
    if constexpr (C::ID != 0) {
      return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "ecgpu_schnorr_sign_prehash_batch: BIP340 is defined over secp256k1 only");
    } else {
      u32 *p_xy, *r_xy, *k;
      int rc = ecgpu_carve(c, c->ecdsa_ws, [&](WsCarver& ws) { p_xy = ws.take<u32>(n * 2 * C::NB); r_xy = ws.take<u32>(n * 2 * C::NB); k = ws.take<u32>(n * C::NB); });
      if (rc) return rc;
      StreamWipe wipe{c, k, n * C::NB};
      const unsigned g = ecgpu_grid_for(c, n, 8);
      if ((rc = mul_gen_ct(c, d, p_xy, FMT_AFFINE, nullptr, n))) return rc;
      hipLaunchKernelGGL((sign::schnorr_nonce_kernel<0>), dim3(g), dim3(256), 0, c->stream, d, (const u32*)p_xy, aux, m, k, n);
      HIPCHK(c, hipGetLastError());
      if ((rc = mul_gen_ct(c, k, r_xy, FMT_AFFINE, nullptr, n))) return rc;
      hipLaunchKernelGGL((sign::schnorr_finish_kernel<0>), dim3(g), dim3(256), 0, c->stream, d, (const u32*)p_xy, (const u32*)k, (const u32*)r_xy, m, sig,
                         pubkeys_x, ok, n);
      HIPCHK(c, hipGetLastError());
      return 0;
    }
  }
  // scalar field (scalar_ops.hpp): element-wise ops one lane per element, inversions SCALAR_INV_BATCH per lane
  static int scalar_op(ecgpu_ctx* c, int op, const u32* a, const u32* b, u32* o, uint8_t* ok, size_t n) {
    using O = OrderOf<C>;
    constexpr int B = SCALAR_INV_BATCH;
    switch (op) {
#define SOP(OPC) case OPC: hipLaunchKernelGGL((scalar_op_kernel<O, OPC>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, a, b, o, ok, n); break;
      SOP(SC_MUL) SOP(SC_SQR) SOP(SC_ADD) SOP(SC_SUB) SOP(SC_NEG) SOP(SC_SQRT)
#undef SOP
      case SC_INV:
        hipLaunchKernelGGL((scalar_inv_kernel<O, B>), dim3(ecgpu_grid_for(c, (n + B - 1) / B, 8)), dim3(256), 0, c->stream, a, o, ok, n);
        break;
      default: return ecgpu_set_err(c, ECGPU_ERR_ARG, "unknown scalar op %d", op);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int scalar_reduce(ecgpu_ctx* c, const uint8_t* in, size_t in_bytes, u32* o, size_t n, unsigned flags) {
    using O = OrderOf<C>;
    const unsigned g = ecgpu_grid_for(c, n, 8);
    if (flags & SC_REDUCE_NONZERO)
      hipLaunchKernelGGL((scalar_reduce_kernel<O, true>), dim3(g), dim3(256), 0, c->stream, in, (int)in_bytes, o, n);
    else
      hipLaunchKernelGGL((scalar_reduce_kernel<O, false>), dim3(g), dim3(256), 0, c->stream, in, (int)in_bytes, o, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  // hash layer (h2c_hash.hpp): one message per lane
  static int h2c_hash_to_field(ecgpu_ctx* c, const uint8_t* msgs, size_t msg_stride, const u32* msg_len, const h2c::XmdTail& tail, int count, u32* u, size_t n) {
    const unsigned g = ecgpu_grid_for(c, n, 8);
    if (count == 2)
      hipLaunchKernelGGL((h2c::hash_to_field_kernel<C, 2>), dim3(g), dim3(256), 0, c->stream, msgs, msg_stride, msg_len, tail, u, n);
    else
      hipLaunchKernelGGL((h2c::hash_to_field_kernel<C, 1>), dim3(g), dim3(256), 0, c->stream, msgs, msg_stride, msg_len, tail, u, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int field_from_okm(ecgpu_ctx* c, const uint8_t* okm, u32* out, size_t n) {
    hipLaunchKernelGGL((h2c::field_from_okm_kernel<C>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, okm, out, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  static int schnorr_challenge(ecgpu_ctx* c, const u32* px, const u32* sig, const u32* prehash, u32* e, size_t n) {
    if constexpr (C::ID != 0) {
      return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "ecgpu_schnorr_verify_prehash_batch: BIP340 is defined over secp256k1 only");
    } else {
      hipLaunchKernelGGL((h2c::bip340_challenge_kernel<0>), dim3(ecgpu_grid_for(c, n, 8)), dim3(256), 0, c->stream, px, sig, prehash, e, n);
      HIPCHK(c, hipGetLastError());
      return 0;
    }
  }
  static const ecgpu_curve_ops* table() {
    static const ecgpu_curve_ops t = {field_op, point_op, point_eq, normalize, lincomb, msm, validate_scalars, validate_points,
                                      decompress, synth_scalars, synth_points, to_bytes, from_bytes, sec1_encode, sec1_decode, ecdsa_verify, h2c_map, ecdsa_recover, schnorr_verify, ecdsa_sign, ecdh,
                                      pass_units, scalar_op, scalar_reduce, h2c_hash_to_field, field_from_okm, schnorr_challenge,
                                      rfc6979_nonce, ecdsa_sign_prehash, schnorr_sign_prehash, schnorr_batch_verify,
                                      shared_table_bytes, shared_build, shared_lincomb, broadcast_points, ecdsa_verify_shared};
    return &t;
  }
};

}  // namespace ecgpu
