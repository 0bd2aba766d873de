// TEST-ONLY gfx950 build of the field and scalar primitives (tests/devtwin/primitive_ops.hpp): the code the kernels run, with
// the inline-asm column forms of mp32_cols.inc, one element per lane.  Checked by tests/test_gpu_field_primitives.py against
// Python integers and against the host twin.  Never linked into libecgpu.so.
//
// Every entry point takes host arrays of raw little-endian 32-bit words, copies them to the device, launches one element per
// lane in blocks of 256, copies the results back, frees, and returns the first HIP error code (0: success, -1: bad argument).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "primitive_ops.hpp"

using namespace ecgpu;
using namespace ecgpu::twin;

namespace {

constexpr int BLOCK = 256;

__global__ void k256_kernel(int op, const u32* a, const u32* b, const u32* e, const u32* f, u32* out, int n) {
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  u32 r[9];
  k256_op(op, a + 8 * i, b + 8 * i, e + 8 * i, f + 8 * i, r);
  for (int w = 0; w < 9; w++) out[9 * i + w] = r[w];
}

template <class M>
__global__ void mont_kernel(int op, const u32* a, const u32* b, u32* out, int n) {
  constexpr int N = M::N;
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  u32 r[N + 1];
  mont_op<M>(op, a + N * i, b + N * i, r);
  for (int w = 0; w <= N; w++) out[(N + 1) * i + w] = r[w];
}

template <class O>
__global__ void scalar_kernel(int op, const u32* a, const u32* b, u32* out, int n) {
  constexpr int L = O::L;
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  u32 r[L];
  scalar_op<O>(op, a + L * i, b + L * i, r);
  for (int w = 0; w < L; w++) out[L * i + w] = r[w];
}

__global__ void mac_kernel(int m, int fresh, int nc, const u32* c_in, const u32* pa, const u32* pb, u32* out, int n) {
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  u32 r[3];
  mac_cols_op(m, fresh, nc, c_in + 3 * i, pa + MAC_MAX_M * i, pb + MAC_MAX_M * i, r);
  for (int w = 0; w < 3; w++) out[3 * i + w] = r[w];
}

// device copies of up to six host arrays; the destructor frees whatever was allocated
struct DevArrays {
  static constexpr int MAXN = 6;
  void* p[MAXN] = {};
  int count = 0;
  ~DevArrays() {
    for (int k = 0; k < count; k++) (void)hipFree(p[k]);
  }
  hipError_t in(const u32*& d, const u32* h, size_t words) {
    void* q = nullptr;
    hipError_t err = hipMalloc(&q, words * sizeof(u32));
    if (err != hipSuccess) return err;
    p[count++] = q;
    d = static_cast<const u32*>(q);
    return hipMemcpy(q, h, words * sizeof(u32), hipMemcpyHostToDevice);
  }
  hipError_t outbuf(u32*& d, size_t words) {
    void* q = nullptr;
    hipError_t err = hipMalloc(&q, words * sizeof(u32));
    if (err != hipSuccess) return err;
    p[count++] = q;
    d = static_cast<u32*>(q);
    return hipMemset(q, 0, words * sizeof(u32));
  }
};

#define DT_CHECK(x)                          \
  do {                                       \
    hipError_t err_ = (x);                   \
    if (err_ != hipSuccess) return (int)err_; \
  } while (0)

int grid(int n) { return (n + BLOCK - 1) / BLOCK; }

// launch, wait, and copy `words` result words back
int finish(u32* host_out, const u32* dev_out, size_t words) {
  DT_CHECK(hipGetLastError());
  DT_CHECK(hipDeviceSynchronize());
  DT_CHECK(hipMemcpy(host_out, dev_out, words * sizeof(u32), hipMemcpyDeviceToHost));
  return 0;
}

template <class M>
int run_mont(int op, const u32* a, const u32* b, u32* out, int n) {
  constexpr size_t N = M::N;
  DevArrays d;
  const u32 *da, *db;
  u32* dout;
  DT_CHECK(d.in(da, a, N * n));
  DT_CHECK(d.in(db, b, N * n));
  DT_CHECK(d.outbuf(dout, (N + 1) * n));
  mont_kernel<M><<<grid(n), BLOCK>>>(op, da, db, dout, n);
  return finish(out, dout, (N + 1) * n);
}

template <class O>
int run_scalar(int op, const u32* a, const u32* b, u32* out, int n) {
  constexpr size_t L = O::L;
  DevArrays d;
  const u32 *da, *db;
  u32* dout;
  DT_CHECK(d.in(da, a, L * n));
  DT_CHECK(d.in(db, b, L * n));
  DT_CHECK(d.outbuf(dout, L * n));
  scalar_kernel<O><<<grid(n), BLOCK>>>(op, da, db, dout, n);
  return finish(out, dout, L * n);
}

}  // namespace

extern "C" {

// op: twin::K256Op.  a, b, e, f: n x 8 words; out: n x 9 words (8 result words, 1 flag word)
int dt_k256_op(int op, const u32* a, const u32* b, const u32* e, const u32* f, u32* out, int n) {
  if (op < 0 || op >= K_NOPS || n < 0 || !a || !b || !e || !f || !out) return -1;
  if (n == 0) return 0;
  DevArrays d;
  const u32 *da, *db, *de, *df;
  u32* dout;
  DT_CHECK(d.in(da, a, 8 * (size_t)n));
  DT_CHECK(d.in(db, b, 8 * (size_t)n));
  DT_CHECK(d.in(de, e, 8 * (size_t)n));
  DT_CHECK(d.in(df, f, 8 * (size_t)n));
  DT_CHECK(d.outbuf(dout, 9 * (size_t)n));
  k256_kernel<<<grid(n), BLOCK>>>(op, da, db, de, df, dout, n);
  return finish(out, dout, 9 * (size_t)n);
}

// curve: 0 P-256, 1 P-384; op: twin::MontOp.  a, b: n x N words; out: n x (N + 1) words
int dt_mont_op(int curve, int op, const u32* a, const u32* b, u32* out, int n) {
  if (op < 0 || op >= M_NOPS || n < 0 || !a || !b || !out) return -1;
  if (n == 0) return 0;
  if (curve == 0) return run_mont<P256Mod>(op, a, b, out, n);
  if (curve == 1) return run_mont<P384Mod>(op, a, b, out, n);
  return -1;
}

// curve: 0 secp256k1, 1 P-256, 2 P-384 (group orders); op: twin::ScalarOp.  a, b, out: n x L words
int dt_scalar_op(int curve, int op, const u32* a, const u32* b, u32* out, int n) {
  if (op < 0 || op >= S_NOPS || n < 0 || !a || !b || !out) return -1;
  if (n == 0) return 0;
  if (curve == 0) return run_scalar<K256Order>(op, a, b, out, n);
  if (curve == 1) return run_scalar<P256Order>(op, a, b, out, n);
  if (curve == 2) return run_scalar<P384Order>(op, a, b, out, n);
  return -1;
}

// mac_cols<m, fresh, nc>: c_in, out: n x 3 words (c.lo low, c.lo high, c.hi); pa, pb: n x 13 words
int dt_mac_cols(int m, int fresh, int nc, const u32* c_in, const u32* pa, const u32* pb, u32* out, int n) {
  if (!mac_cols_valid(m, fresh, nc) || n < 0 || !c_in || !pa || !pb || !out) return -1;
  if (n == 0) return 0;
  DevArrays d;
  const u32 *dc, *dpa, *dpb;
  u32* dout;
  DT_CHECK(d.in(dc, c_in, 3 * (size_t)n));
  DT_CHECK(d.in(dpa, pa, MAC_MAX_M * (size_t)n));
  DT_CHECK(d.in(dpb, pb, MAC_MAX_M * (size_t)n));
  DT_CHECK(d.outbuf(dout, 3 * (size_t)n));
  mac_kernel<<<grid(n), BLOCK>>>(m, fresh, nc, dc, dpa, dpb, dout, n);
  return finish(out, dout, 3 * (size_t)n);
}

}  // extern "C"
