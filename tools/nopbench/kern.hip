// Device side of the s_nop cost experiment: a dependent chain of k256 multiplications / squarings per lane.
// KERN_EXACT: the exact columns (every product with its carry addition, k256::mul_exact / sqr_exact) instead of the library's
// speculative ones: the A/B of profiles/spec_carry.txt.
#include "fe_k256.hpp"
#ifdef KERN_EXACT
#define KMUL k256::mul_exact
#define KSQR k256::sqr_exact
#else
#define KMUL k256::mul
#define KSQR k256::sqr
#endif
#ifndef KWAVES
#define KWAVES 4
#endif
using namespace ecgpu;
extern "C" __global__ void __launch_bounds__(256, KWAVES) kloop(const u32* a, const u32* b, u32* o, int iters) {
  FeK256 x, y, r;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int i = 0; i < 8; i++) { x.v[i] = a[t * 8 + i]; y.v[i] = b[t * 8 + i]; }
  r = x;
#pragma unroll 1
  for (int it = 0; it < iters; it++) {
    KMUL(r, r, y);
    KSQR(x, r);
    KMUL(r, x, r);
    k256::add(y, y, x);
  }
  for (int i = 0; i < 8; i++) o[t * 8 + i] = r.v[i];
}
