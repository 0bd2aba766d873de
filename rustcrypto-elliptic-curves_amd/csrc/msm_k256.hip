// Pippenger MSM for k256: msm_kernels.hpp instantiated in its own translation unit (the library builds in parallel).
// ECGPU_K256_EXACT_PRODUCTS: the bucket kernels keep the field products with every carry addition (fe_k256.hpp).  With the speculative
// columns the 2^23-pair MSM measured about 3 % slower (profiles/spec_carry.txt), while the variable-base kernels gain.
#define ECGPU_K256_EXACT_PRODUCTS 1
#include "msm_kernels.hpp"
using namespace ecgpu;
static_assert(2 * ECGPU_SCHNORR_BATCH_MIN + 1 >= msm::SMALL_MSM_TERMS, "the batch equation's default crossover lies at or above the MSM's small-sum limit");
int ecgpu_msm_k256(ecgpu_ctx* c, const uint32_t* sc, const uint32_t* pts, int pt_fmt, size_t n, uint32_t* out, int out_fmt, ecgpu_msm_mul_fn mul) {
  return msm::msm_run<CurveK256>(c, sc, pts, pt_fmt, n, out, out_fmt, [&](const u32* s, const u32* p, int fmt, u32* prod, size_t cnt) { return mul(c, s, p, fmt, prod, cnt); });
}
