// TEST-ONLY host build of the scalar fields (scalar_mont.hpp: smont::mul / add / reduce_once / to_mont / from_mont / inv for
// the three group orders), with the op table of the device twin (tests/devtwin/primitive_ops.hpp).  Checked against Python
// integers by tests/test_hosttwin_scalar_field.py.
#include "hosttwin_trace.hpp"
#include "../devtwin/primitive_ops.hpp"
using namespace ecgpu;
using namespace ecgpu::twin;

template <class O>
static int scalar_rows(int op, const u32* a, const u32* b, u32* out, int n) {
  constexpr int L = O::L;
  for (int i = 0; i < n; i++)
    if (!scalar_op<O>(op, a + L * i, b + L * i, out + L * i)) return -1;
  return 0;
}

extern "C" {
// curve: 0 secp256k1, 1 P-256, 2 P-384 (group orders); op: twin::ScalarOp.  a, b, out: n x L little-endian 32-bit words
int ht_scalar_op(int curve, int op, const u32* a, const u32* b, u32* out, int n) {
  if (curve == 0) return scalar_rows<K256Order>(op, a, b, out, n);
  if (curve == 1) return scalar_rows<P256Order>(op, a, b, out, n);
  if (curve == 2) return scalar_rows<P384Order>(op, a, b, out, n);
  return -1;
}
}
