// TEST-ONLY gfx950 build of the RFC 6979 nonce generator (csrc/hmac_drbg.hpp), one rfc6979::generate_k per lane with the order q
// given by the caller, so that a modulus that rejects often drives the rejection loop (step h.3) on the device: lanes of one wave
// leave the loop at different rounds.  Checked by tests/test_gpu_group_edges.py against tests/rfc6979_model.py and the host twin.
// An object of its own: the two configurations of the point formulas (devtwin_group.hip) do not need it.  Never linked into libecgpu.so.
#include "hmac_drbg.hpp"
#include "devtwin_launch.hpp"

using namespace ecgpu;
using namespace ecgpu::twin;

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_LANES = 1 << 13;

// x, h1, k: NW little-endian limbs per lane; extra: NW limbs and a presence word per lane (non-zero: the lane runs the EXTRA form)
template <class H, int NW>
__global__ void generate_k_kernel(const u32* x, const u32* h1, const u32* extra, const u32* q, u32* k, u32* rejected, int n) {
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  u32 xl[NW], hl[NW], el[NW], ql[NW], kl[NW];
  for (int w = 0; w < NW; w++) {
    xl[w] = x[NW * i + w];
    hl[w] = h1[NW * i + w];
    el[w] = extra ? extra[(NW + 1) * i + w] : 0u;
    ql[w] = q[w];
  }
  int rej;
  if (extra && extra[(NW + 1) * i + NW]) rej = rfc6979::generate_k<H, NW, true>(kl, xl, hl, el, ql);
  else rej = rfc6979::generate_k<H, NW, false>(kl, xl, hl, nullptr, ql);
  for (int w = 0; w < NW; w++) k[NW * i + w] = kl[w];
  rejected[i] = (u32)rej;
}

template <class H, int NW>
int run(const u32* x, const u32* h1, const u32* extra, const u32* q, u32* k, u32* rejected, int n) {
  DevArrays d;
  const u32 *dx, *dh, *de = nullptr, *dq;
  u32 *dk, *dr;
  DT_CHECK(d.in(dx, x, (size_t)NW * n));
  DT_CHECK(d.in(dh, h1, (size_t)NW * n));
  if (extra) DT_CHECK(d.in(de, extra, (size_t)(NW + 1) * n));
  DT_CHECK(d.in(dq, q, NW));
  DT_CHECK(d.outbuf(dk, (size_t)NW * n));
  DT_CHECK(d.outbuf(dr, n));
  generate_k_kernel<H, NW><<<(n + BLOCK - 1) / BLOCK, BLOCK>>>(dx, dh, de, dq, dk, dr, n);
  DT_CHECK(hipGetLastError());
  DT_CHECK(hipDeviceSynchronize());
  DT_CHECK(hipMemcpy(k, dk, (size_t)NW * n * sizeof(u32), hipMemcpyDeviceToHost));
  DT_CHECK(hipMemcpy(rejected, dr, (size_t)n * sizeof(u32), hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" {

// hash: 0 SHA-256 (NW = 8), 1 SHA-384 (NW = 12).  x, h1, k: n x NW words; extra: NULL, or n x (NW + 1) words, the last one of a
// row saying whether that lane has additional data; q: NW words, 2^(32 NW - 1) <= q (a candidate is then rejected with
// probability below 1/2 and the loop ends); rejected: n words.  At most 2^13 lanes per call.
int dt_rfc6979_generate_k(int hash, const u32* x, const u32* h1, const u32* extra, const u32* q, u32* k, u32* rejected, int n) {
  if (n < 0 || n > MAX_LANES || !x || !h1 || !q || !k || !rejected) return -1;
  if (hash != 0 && hash != 1) return -1;
  if (!(q[(hash == 0 ? 8 : 12) - 1] >> 31)) return -1;
  if (n == 0) return 0;
  if (hash == 0) return run<sha2::Sha256, 8>(x, h1, extra, q, k, rejected, n);
  return run<sha2::Sha384, 12>(x, h1, extra, q, k, rejected, n);
}

}  // extern "C"
