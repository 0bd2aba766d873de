// TEST-ONLY gfx950 build of the point formulas and the masked additions (tests/devtwin/group_ops.hpp): the code the kernels run,
// one pair of operands per lane, so that the lanes of a wave can take different branches of one formula.  Checked by
// tests/test_gpu_group_edges.py against Python integers and against the host twin.  Never linked into libecgpu.so.
//
// The entry point takes host arrays of raw little-endian 32-bit words, copies them to the device, launches one pair per lane in
// blocks of 256, copies the results back, frees, and returns the first HIP error code (0: success, -1: bad argument).
#include "group_ops.hpp"
#include "devtwin_launch.hpp"

using namespace ecgpu;
using namespace ecgpu::twin;

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_PAIRS = 1 << 13;

template <class C>
__global__ void pt_kernel(int op, const u32* p, const u32* q, const u32* aux, u32* out, int n) {
  constexpr int IN = PT_IN_FE * C::NW, OUT = pt_out_words<C>();
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  u32 r[OUT];
  pt_op<C>(op, p + IN * i, q + IN * i, aux + PT_AUX * i, r);
  for (int w = 0; w < OUT; w++) out[OUT * i + w] = r[w];
}

template <class C>
int run_pt(int op, const u32* p, const u32* q, const u32* aux, u32* out, int n) {
  constexpr size_t IN = PT_IN_FE * C::NW, OUT = pt_out_words<C>();
  DevArrays d;
  const u32 *dp, *dq, *da;
  u32* dout;
  DT_CHECK(d.in(dp, p, IN * n));
  DT_CHECK(d.in(dq, q, IN * n));
  DT_CHECK(d.in(da, aux, (size_t)PT_AUX * n));
  DT_CHECK(d.outbuf(dout, OUT * n));
  pt_kernel<C><<<(n + BLOCK - 1) / BLOCK, BLOCK>>>(op, dp, dq, da, dout, n);
  DT_CHECK(hipGetLastError());
  DT_CHECK(hipDeviceSynchronize());
  DT_CHECK(hipMemcpy(out, dout, OUT * n * sizeof(u32), hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" {

// curve: 0 secp256k1, 1 P-256, 2 P-384; op: twin::PtOp.  p, q: n x 4 NW words; aux: n x 2 words; out: n x (5 NW + 1) words.
// At most 2^13 pairs per call.
int dt_pt_op(int curve, int op, const u32* p, const u32* q, const u32* aux, u32* out, int n) {
  if (op < 0 || op >= PT_NOPS || n < 0 || n > MAX_PAIRS || !p || !q || !aux || !out) return -1;
  if (op >= K_JAC_ADD_MIXED && curve != 0) return -1;
  if (op == M_VBCT_ACCUMULATE && curve == 0) return -1;
  if (n == 0) return 0;
  if (curve == 0) return run_pt<CurveK256>(op, p, q, aux, out, n);
  if (curve == 1) return run_pt<CurveP256>(op, p, q, aux, out, n);
  if (curve == 2) return run_pt<CurveP384>(op, p, q, aux, out, n);
  return -1;
}

}  // extern "C"
