// TEST-ONLY gfx950 build of the two ECDSA kernels whose x(R) >= n arms the C ABI cannot reach with chosen inputs
// (csrc/ecdsa_kernels.hpp, launched unchanged): sign_finish_kernel with R given, not computed from k, so that R can lie at a chosen x in
// [n, p) - x_reduced, r = x - n and bit 1 of the recovery id; and verify_check_kernel with the two products A and B given, so that the
// tangent A = B and either operand at infinity meet the second candidate r + n.  Checked by tests/test_gpu_ecdsa_wrap.py against the
// models of tests/ecdsa_wrap_vectors.py.  Never linked into libecgpu.so.
//
// The entry points take host arrays in the kernels' own layout - the ABI's rows of big-endian bytes, flags one byte per row - copy
// them to the device, launch with the product's grid (256-thread workgroups; sign_finish: 16 rows per lane, one workgroup up to 4096
// rows; verify_check: one row per lane), copy the results back, free, and return the first HIP error code (0: success, -1: bad argument).
#include "ecdsa_kernels.hpp"
#include "devtwin_launch.hpp"

using namespace ecgpu;
using namespace ecgpu::twin;

namespace {

constexpr int BLOCK = 256;
constexpr int SIGN_BATCH = 16;
constexpr int MAX_ROWS = 1 << 13;

const u32* words(const uint8_t* p) { return reinterpret_cast<const u32*>(p); }

template <class C>
int run_sign_finish(const uint8_t* d, const uint8_t* k, const uint8_t* z, const uint8_t* r_xy, const uint8_t* r_inf, unsigned flags, uint8_t* sig,
                    uint8_t* recid, uint8_t* ok, int n) {
  constexpr size_t L = C::NW;
  DevArrays a;
  const u32 *dd, *dk, *dz, *dr;
  const uint8_t* dinf;
  u32* dsig;
  uint8_t *drec, *dok;
  DT_CHECK(a.in(dd, words(d), L * n));
  DT_CHECK(a.in(dk, words(k), L * n));
  DT_CHECK(a.in(dz, words(z), L * n));
  DT_CHECK(a.in(dr, words(r_xy), 2 * L * n));
  DT_CHECK(a.in_bytes(dinf, r_inf, n));
  DT_CHECK(a.outbuf(dsig, 2 * L * n));
  DT_CHECK(a.outbuf_bytes(drec, n));
  DT_CHECK(a.outbuf_bytes(dok, n));
  const int units = (n + SIGN_BATCH - 1) / SIGN_BATCH;
  ecdsa::sign_finish_kernel<C, SIGN_BATCH><<<(units + BLOCK - 1) / BLOCK, BLOCK>>>(dd, dk, dz, dr, dinf, dsig, drec, dok, (size_t)n, flags);
  DT_CHECK(hipGetLastError());
  DT_CHECK(hipDeviceSynchronize());
  DT_CHECK(hipMemcpy(sig, dsig, 2 * L * n * sizeof(u32), hipMemcpyDeviceToHost));
  DT_CHECK(hipMemcpy(recid, drec, n, hipMemcpyDeviceToHost));
  DT_CHECK(hipMemcpy(ok, dok, n, hipMemcpyDeviceToHost));
  return 0;
}

template <class C>
int run_verify_check(const uint8_t* a_xy, const uint8_t* a_inf, const uint8_t* b_xy, const uint8_t* b_inf, const uint8_t* sig, uint8_t* ok, int n) {
  constexpr size_t L = C::NW;
  DevArrays a;
  const u32 *da, *db, *dsig;
  const uint8_t *dai, *dbi;
  uint8_t* dok;
  DT_CHECK(a.in(da, words(a_xy), 2 * L * n));
  DT_CHECK(a.in_bytes(dai, a_inf, n));
  DT_CHECK(a.in(db, words(b_xy), 2 * L * n));
  DT_CHECK(a.in_bytes(dbi, b_inf, n));
  DT_CHECK(a.in(dsig, words(sig), 2 * L * n));
  DT_CHECK(a.outbuf_bytes(dok, n));
  DT_CHECK(hipMemcpy(dok, ok, n, hipMemcpyHostToDevice));
  ecdsa::verify_check_kernel<C><<<(n + BLOCK - 1) / BLOCK, BLOCK>>>(da, dai, db, dbi, dsig, dok, (size_t)n);
  DT_CHECK(hipGetLastError());
  DT_CHECK(hipDeviceSynchronize());
  DT_CHECK(hipMemcpy(ok, dok, n, hipMemcpyDeviceToHost));
  return 0;
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" {

// curve: 0 secp256k1, 1 P-256, 2 P-384, NB = 32, 32, 48 bytes.  d, k, z: n x NB; r_xy: n x 2 NB (x || y of R); r_inf: n bytes (non-zero:
// R is the identity); flags: the ABI's (ECGPU_ECDSA_LOW_S = 2).  Out: sig n x 2 NB (r || s), recid and ok n bytes.  The multi-byte
// arrays 4-byte aligned; at most 2^13 rows per call.
int dt_ecdsa_sign_finish(int curve, const uint8_t* d, const uint8_t* k, const uint8_t* z, const uint8_t* r_xy, const uint8_t* r_inf, unsigned flags,
                         uint8_t* sig, uint8_t* recid, uint8_t* ok, int n) {
  if (n < 0 || n > MAX_ROWS || !d || !k || !z || !r_xy || !r_inf || !sig || !recid || !ok) return -1;
  if (!aligned4(d) || !aligned4(k) || !aligned4(z) || !aligned4(r_xy) || !aligned4(sig)) return -1;
  if (n == 0) return 0;
  if (curve == 0) return run_sign_finish<CurveK256>(d, k, z, r_xy, r_inf, flags, sig, recid, ok, n);
  if (curve == 1) return run_sign_finish<CurveP256>(d, k, z, r_xy, r_inf, flags, sig, recid, ok, n);
  if (curve == 2) return run_sign_finish<CurveP384>(d, k, z, r_xy, r_inf, flags, sig, recid, ok, n);
  return -1;
}

// a_xy, b_xy: n x 2 NB (the products A = u1 G and B = u2 Q, affine); a_inf, b_inf: n bytes; sig: n x 2 NB (only r is read);
// ok: n bytes, in (0: rejected before, stays 0) and out.
int dt_ecdsa_verify_check(int curve, const uint8_t* a_xy, const uint8_t* a_inf, const uint8_t* b_xy, const uint8_t* b_inf, const uint8_t* sig,
                          uint8_t* ok, int n) {
  if (n < 0 || n > MAX_ROWS || !a_xy || !a_inf || !b_xy || !b_inf || !sig || !ok) return -1;
  if (!aligned4(a_xy) || !aligned4(b_xy) || !aligned4(sig)) return -1;
  if (n == 0) return 0;
  if (curve == 0) return run_verify_check<CurveK256>(a_xy, a_inf, b_xy, b_inf, sig, ok, n);
  if (curve == 1) return run_verify_check<CurveP256>(a_xy, a_inf, b_xy, b_inf, sig, ok, n);
  if (curve == 2) return run_verify_check<CurveP384>(a_xy, a_inf, b_xy, b_inf, sig, ok, n);
  return -1;
}

}  // extern "C"
