// TEST-ONLY host build of the point-formula op table (tests/devtwin/group_ops.hpp): the functions tests/devtwin/devtwin_group.hip
// runs one pair per lane, here one pair after the other with the ECGPU_EXC_NOTE counters on (ht_exc_reset / ht_exc_counts), so that
// tests/test_hosttwin_group_edges.py can show which branch each class of tests/group_edge_vectors.py reaches.
#include "hosttwin_trace.hpp"
#include "../devtwin/group_ops.hpp"
using namespace ecgpu;
using namespace ecgpu::twin;

template <class C>
static int run_pt(int op, const u32* p, const u32* q, const u32* aux, u32* out, int n) {
  constexpr size_t IN = PT_IN_FE * C::NW, OUT = pt_out_words<C>();
  for (int i = 0; i < n; i++)
    if (!pt_op<C>(op, p + IN * i, q + IN * i, aux + PT_AUX * i, out + OUT * i)) return -1;
  return 0;
}

// the arguments of dt_pt_op (tests/devtwin/devtwin_group.hip)
extern "C" int ht_pt_op(int curve, int op, const u32* p, const u32* q, const u32* aux, u32* out, int n) {
  if (op < 0 || op >= PT_NOPS || n < 0 || !p || !q || !aux || !out) return -1;
  if (curve == 0) return run_pt<CurveK256>(op, p, q, aux, out, n);
  if (curve == 1) return run_pt<CurveP256>(op, p, q, aux, out, n);
  if (curve == 2) return run_pt<CurveP384>(op, p, q, aux, out, n);
  return -1;
}
