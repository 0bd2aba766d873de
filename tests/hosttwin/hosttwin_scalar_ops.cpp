// TEST-ONLY host build of the scalar-field ops (scalar_ops.hpp: the element-wise ops, the masked batched inversion and the
// wide / nonzero reductions) for the three group orders.  Checked against Python integers by tests/test_hosttwin_scalar_ops.py.
#include "hosttwin_trace.hpp"
#include "scalar_ops.hpp"
using namespace ecgpu;

template <class O>
static int op_rows(int op, const u32* a, const u32* b, u32* out, uint8_t* ok, int n) {
  constexpr int L = O::L;
  for (int i = 0; i < n; i++) {
    const u32 *x = a + L * i, *y = b + L * i;
    u32* r = out + L * i;
    u32 g;
    switch (op) {
      case SC_MUL: g = scops::elem<O, SC_MUL>(r, x, y); break;
      case SC_SQR: g = scops::elem<O, SC_SQR>(r, x, y); break;
      case SC_ADD: g = scops::elem<O, SC_ADD>(r, x, y); break;
      case SC_SUB: g = scops::elem<O, SC_SUB>(r, x, y); break;
      case SC_NEG: g = scops::elem<O, SC_NEG>(r, x, y); break;
      case SC_SQRT: g = scops::elem<O, SC_SQRT>(r, x, y); break;
      default: return -1;
    }
    ok[i] = (uint8_t)g;
  }
  return 0;
}
template <class O, int BATCH>
static int inv_lane_rows(const u32* a, int cnt, u32* out, uint8_t* ok) {
  constexpr int L = O::L;
  if (cnt < 1 || cnt > BATCH) return -1;
  u32 v[BATCH][L];
  for (int b = 0; b < cnt; b++) mp_copy<L>(v[b], a + L * b);
  const u32 good = scops::inv_lane<O, BATCH>(v, cnt);
  for (int b = 0; b < cnt; b++) {
    mp_copy<L>(out + L * b, v[b]);
    ok[b] = (uint8_t)((good >> b) & 1u);
  }
  return 0;
}
template <class O>
static int inv_lane_any(int batch, const u32* a, int cnt, u32* out, uint8_t* ok) {
  switch (batch) {
    case 1: return inv_lane_rows<O, 1>(a, cnt, out, ok);
    case 8: return inv_lane_rows<O, 8>(a, cnt, out, ok);
    case 16: return inv_lane_rows<O, 16>(a, cnt, out, ok);
    case 32: return inv_lane_rows<O, 32>(a, cnt, out, ok);
    default: return -1;
  }
}
template <class O>
static int reduce_rows(int nonzero, const uint8_t* in, int in_bytes, u32* out, int n) {
  constexpr int L = O::L;
  if (in_bytes < 1 || in_bytes > 8 * L) return -1;
  for (int i = 0; i < n; i++) {
    u32 w[2 * L];
    scops::load_wide<O>(w, in + (size_t)in_bytes * i, in_bytes);
    if (nonzero) scops::reduce_nonzero<O>(out + L * i, w);
    else scops::reduce_wide<O>(out + L * i, w);
  }
  return 0;
}

extern "C" {
// curve: 0 secp256k1, 1 P-256, 2 P-384 (group orders); a, b, out: n x L little-endian 32-bit words
int ht_sc_op(int curve, int op, const u32* a, const u32* b, u32* out, uint8_t* ok, int n) {
  if (curve == 0) return op_rows<K256Order>(op, a, b, out, ok, n);
  if (curve == 1) return op_rows<P256Order>(op, a, b, out, ok, n);
  if (curve == 2) return op_rows<P384Order>(op, a, b, out, ok, n);
  return -1;
}
// one lane of scalar_inv_kernel: cnt (1 .. batch) elements, batch one of 1, 8, 16, 32
int ht_sc_inv_lane(int curve, int batch, const u32* a, int cnt, u32* out, uint8_t* ok) {
  if (curve == 0) return inv_lane_any<K256Order>(batch, a, cnt, out, ok);
  if (curve == 1) return inv_lane_any<P256Order>(batch, a, cnt, out, ok);
  if (curve == 2) return inv_lane_any<P384Order>(batch, a, cnt, out, ok);
  return -1;
}
int ht_sc_inv_default_batch(void) { return SCALAR_INV_BATCH; }
// n big-endian records of in_bytes bytes -> n x L little-endian words
int ht_sc_reduce(int curve, int nonzero, const uint8_t* in, int in_bytes, u32* out, int n) {
  if (curve == 0) return reduce_rows<K256Order>(nonzero, in, in_bytes, out, n);
  if (curve == 1) return reduce_rows<P256Order>(nonzero, in, in_bytes, out, n);
  if (curve == 2) return reduce_rows<P384Order>(nonzero, in, in_bytes, out, n);
  return -1;
}
// the fold constants of the nonzero reduction (tests recompute them and the bound of NF folds)
int ht_sc_fold_params(int curve, u32* c, int* cw, int* nf) {
  auto put = [&](auto aux) {
    using A = decltype(aux);
    for (int i = 0; i < A::CW; i++) c[i] = A::C[i];
    *cw = A::CW;
    *nf = A::NF;
  };
  if (curve == 0) put(ScalarAux<K256Order>{});
  else if (curve == 1) put(ScalarAux<P256Order>{});
  else if (curve == 2) put(ScalarAux<P384Order>{});
  else return -1;
  return 0;
}
}
