// Kernels and launchers of one NIST curve (included by ops_p256.hip and ops_p384.hip with ECGPU_NIST_CURVE and
// ECGPU_NIST_OPS_FN defined: one translation unit per curve so that the library builds in parallel, one source).
#include "curve_ops.hpp"
#include "varbase.hpp"
#ifndef VBB
#define VBB 16         // units per lane and pass of the variable-base kernels (their tables and their results share one inversion each).
#endif                 // Round 3, 2^22 units, 8 -> 16: P-384 250.5 -> 248.6 ms, P-256 77.5 -> 77.1 ms (the inversion's share halves; the workspace doubles)
// window width of the single-term variable-base kernel: 4 or 5 bits (varbase_lane.hpp).  Round 4, 2^22 units, alternating passes: P-384
// 243.2-244.0 ms with 4-bit windows, 236.6-237.1 ms with 5-bit windows (-2.8 %: 77 windows and 16 table entries instead of 97 and 8); P-256
// 75.8-76.1 against 76.4-76.8 ms (its additions are cheaper relative to a table entry): 5 bits for the 12-word field only
// (profiles/r04_ab_measurements.txt, set three)
#ifndef VB_WINDOW
#define VB_WINDOW(C) ((C::NW > 8) ? 5 : 4)
#endif
// per-lane units a wave draws at a time (sched.hpp): the units of one draw share the inversion of their tables (~400 multiplications on P-384, a tenth of
// a unit), the results of up to VBB units share the output inversion
#ifndef VB_CHUNK_UNITS
#define VB_CHUNK_UNITS 2      // P-384, 2^22 units: 1 / 2 / 3 / 4 / 8 / 16 units per draw = 229.6 / 225.5 / 226.1 / 228.1 / 237.4 / 243.0 ms (16 = the static assignment); P-256 73.9-74.2 against 74.0-74.4 at 4
#endif
// a chunk of 0 units never advances the work counter (the kernel hangs: the two-term launch draws VB_CHUNK_UNITS / 2, which is 0 for 1); a chunk above
// the VBB / terms units a lane buffers overruns its result buffer before the flush test
static_assert(VB_CHUNK_UNITS >= 1 && VB_CHUNK_UNITS <= VBB, "one term: VB_CHUNK_UNITS must lie in 1 .. VBB");
static_assert(VB_CHUNK_UNITS / 2 >= 1 && VB_CHUNK_UNITS / 2 <= VBB / 2, "two terms: VB_CHUNK_UNITS / 2 must lie in 1 .. VBB / 2 (VB_CHUNK_UNITS = 1 hangs the kernel)");
#ifndef VB_WAVES
#define VB_WAVES 4     // occupancy target of the public-data variable-base kernels (waves per SIMD): 3 measured equal (P-384) or 2 % worse (P-256)
#endif
// the constant-time kernel keeps every addition's operands live through the masked selects: P-384 gains 3.3 % at 3 waves per
// SIMD (168 VGPRs: 255.1 against 263.7 ms per 2^22), P-256 loses 2 %
#ifndef VBCT_WAVES
#define VBCT_WAVES(C) ((C::NW > 8) ? 3 : VB_WAVES)
#endif
using namespace ecgpu;

template <>
int CurveOps<ECGPU_NIST_CURVE>::lincomb_fast(ecgpu_ctx* c, const u32* sc, const u32* pts, int pt_fmt, size_t terms, u32* out, int out_fmt, uint8_t* out_inf,
                                             size_t n) {
  using C = ECGPU_NIST_CURVE;
  if (terms == 1 && !pts) return mul_gen_fast(c, sc, out, out_fmt, out_inf, n);
  if ((terms == 1 || terms == 2) && pts) {
    // 4 waves per SIMD (128 VGPRs): measured best against 2 and 3 for both curves (round 1)
    const dim3 grid(ecgpu_grid_for(c, n, VB_WAVES));
    // per-lane workspace (VBB tables of 8 points and the prefix products of their shared inversion per resident lane),
    // grow-only, shared with the other curves' kernels
    constexpr int WB = VB_WINDOW(C);
    int rc = ecgpu_reserve(c, c->tab_ws, (size_t)grid.x * 256 * (terms == 2 ? sizeof(vb::LaneWs<C, VBB>) : sizeof(vb::LaneWs<C, VBB, WB>)));
    if (rc) return rc;
    unsigned long long* ctr = ecgpu_sched_counter(c);
    if (!ctr) return ECGPU_ERR_RUNTIME;
    const WaveSched sched{ctr, (unsigned long long)n, grid.x * 4u, (unsigned)(terms == 2 ? VB_CHUNK_UNITS / 2 : VB_CHUNK_UNITS), 1u};
    if (terms == 2)
      hipLaunchKernelGGL((vb::mul_kernel<C, VBB, VB_WAVES, 2>), grid, dim3(256), 0, c->stream, sc, pts, pt_fmt, out, out_fmt, out_inf, n, (vb::LaneWs<C, VBB>*)c->tab_ws.p,
                         sched);
    else
      hipLaunchKernelGGL((vb::mul_kernel<C, VBB, VB_WAVES, 1, WB>), grid, dim3(256), 0, c->stream, sc, pts, pt_fmt, out, out_fmt, out_inf, n,
                         (vb::LaneWs<C, VBB, WB>*)c->tab_ws.p, sched);
    HIPCHK(c, hipGetLastError());
    return 1;
  }
  return 0;   // lincomb with more than two terms: one reference multiplication per term
}
// k P for secret scalars (ECDH): constant-time schedule of varbase_ct.hpp, VBB units per lane and pass
template <>
int CurveOps<ECGPU_NIST_CURVE>::mul_ct(ecgpu_ctx* c, const u32* sc, const u32* pts, int pt_fmt, u32* out, int out_fmt, uint8_t* out_inf, size_t n) {
  using C = ECGPU_NIST_CURVE;
  constexpr int WAVES = VBCT_WAVES(C);
  // more workgroups than the chip holds, STATIC work per workgroup: the hardware hands the waiting workgroups out as the favoured waves of a SIMD leave
  // (sched.hpp explains the imbalance; the constant-time kernels do not draw their work from a counter: their instruction counts stay deterministic)
#ifndef VBCT_GRID_MULT
#define VBCT_GRID_MULT 2         // 2^22 units, 1 / 2 / 4: P-384 250.8 / 238.3 / 235.8 ms, P-256 77.8 / 76.1 / 75.7 ms; 2 keeps the workspace at 6.7 / 7.5 GB
#endif
  const dim3 grid(ecgpu_grid_for(c, n, WAVES * VBCT_GRID_MULT));
  const size_t ws_need = (size_t)grid.x * 256 * vbct::lane_chunks<C, VBB>() * sizeof(vbct::Chunk);
  int rc = ecgpu_reserve(c, c->tab_ws, ws_need);
  if (rc) return rc;
  hipLaunchKernelGGL((vbct::mul_kernel<C, VBB, WAVES>), grid, dim3(256), 0, c->stream, sc, pts, pt_fmt, out, out_fmt, out_inf, n, (vbct::Chunk*)c->tab_ws.p);
  HIPCHK(c, hipGetLastError());
  return 1;
}
template <>
size_t CurveOps<ECGPU_NIST_CURVE>::pass_units_points(const ecgpu_ctx* c, size_t terms, unsigned flags) {
  using C = ECGPU_NIST_CURVE;
  if (flags & ECGPU_EXACT_REFERENCE) return resident_lanes(c, 4);
  if (flags & ECGPU_SECRET_SCALARS) return resident_lanes(c, VBCT_WAVES(C)) * VBB;
  if (terms == 2) return resident_lanes(c, VB_WAVES) * (VBB / 2);
  if (terms > 2) return resident_lanes(c, 4);
  return resident_lanes(c, VB_WAVES) * VBB;
}
// Pippenger MSM (msm.hpp, msm_kernels.hpp; instantiated in msm_p256.hip / msm_p384.hip): no endomorphism on these curves,
// 16 / 24 windows of one scalar
static int nist_mul_for_msm(ecgpu_ctx* c, const u32* s, const u32* p, int fmt, u32* prod, size_t cnt) {
  return CurveOps<ECGPU_NIST_CURVE>::lincomb(c, s, p, fmt, 1, prod, FMT_AFFINE, nullptr, cnt, 0);
}
template <>
int CurveOps<ECGPU_NIST_CURVE>::msm(ecgpu_ctx* c, const u32* sc, const u32* pts, int pt_fmt, size_t n, u32* out, int out_fmt) {
  return ECGPU_NIST_MSM_FN(c, sc, pts, pt_fmt, n, out, out_fmt, nist_mul_for_msm);
}
const ecgpu_curve_ops* ECGPU_NIST_OPS_FN() { return CurveOps<ECGPU_NIST_CURVE>::table(); }
