// TEST-ONLY host build of the k256 / Montgomery field op tables and the column forms (tests/devtwin/primitive_ops.hpp), the
// portable counterpart of tests/devtwin: tests/test_gpu_field_primitives.py requires the device results to be bit-identical.
// Same arguments and word layout as the dt_* entry points of tests/devtwin/devtwin.hip.
#include "hosttwin_trace.hpp"
#include "../devtwin/primitive_ops.hpp"
using namespace ecgpu;
using namespace ecgpu::twin;

template <class M>
static int mont_rows(int op, const u32* a, const u32* b, u32* out, int n) {
  constexpr int N = M::N;
  for (int i = 0; i < n; i++)
    if (!mont_op<M>(op, a + N * i, b + N * i, out + (N + 1) * i)) return -1;
  return 0;
}

extern "C" {
int ht_k256_prim_op(int op, const u32* a, const u32* b, const u32* e, const u32* f, u32* out, int n) {
  for (int i = 0; i < n; i++)
    if (!k256_op(op, a + 8 * i, b + 8 * i, e + 8 * i, f + 8 * i, out + 9 * i)) return -1;
  return 0;
}
int ht_mont_prim_op(int curve, int op, const u32* a, const u32* b, u32* out, int n) {
  if (curve == 0) return mont_rows<P256Mod>(op, a, b, out, n);
  if (curve == 1) return mont_rows<P384Mod>(op, a, b, out, n);
  return -1;
}
int ht_mac_cols(int m, int fresh, int nc, const u32* c_in, const u32* pa, const u32* pb, u32* out, int n) {
  if (!mac_cols_valid(m, fresh, nc)) return -1;
  for (int i = 0; i < n; i++)
    if (!mac_cols_op(m, fresh, nc, c_in + 3 * i, pa + MAC_MAX_M * i, pb + MAC_MAX_M * i, out + 3 * i)) return -1;
  return 0;
}
}
