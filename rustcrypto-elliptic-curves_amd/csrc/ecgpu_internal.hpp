// Shared by the API translation unit (ecgpu.hip) and the per-curve kernel translation units
// (ops_*.hip): context layout, error helpers and the table of kernel launchers of one curve.
// Each curve's kernels are compiled in their own translation unit so the library builds in parallel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <mutex>
#include <vector>

#include "../../include/ecgpu.h"
#include "ws_carver.hpp"
#include "xmd_tail.hpp"

// A grow-only device buffer (ecgpu_reserve below): scratch whose contents do not survive growing.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};
// generator tables of a curve, built on first use (curve_ops.hpp)
enum ecgpu_table_kind {
  ECGPU_TAB_GEN,      // the reference schedule's table
  ECGPU_TAB_FB8,      // fixed-base tables of the throughput schedule (fixedbase.hpp): 8-bit windows
  ECGPU_TAB_FB16,     // 16-bit-window variant for large batches
  ECGPU_TAB_FB20,     // 20-bit-window variant for very large batches
  ECGPU_TAB_FB24,     // 24-bit windows (5.9 GB for a 256-bit curve): batches of 2^23 and more
  ECGPU_TAB_FB26,     // 26-bit windows (21.5 GB): batches of 2^24 and more on the 256-bit curves
  ECGPU_TAB_FBCT,     // 5-bit windows, read in full by the constant-time kernel (signing)
  ECGPU_TAB_COUNT_
};

// terms of one shared-points call that can run from tables (fb::SHARED_MAX_TERMS, sharedbase.hpp: curve_ops.hpp asserts they agree)
constexpr int ECGPU_SHARED_MAX_TERMS = 8;

struct ecgpu_ctx {
  int device = -1;
  int num_cus = 0;
  hipStream_t own_stream = nullptr;           // blocking stream: ordered with the legacy default stream like any ordinary stream
  hipStream_t stream = nullptr;               // where launches go; nullptr is a legitimate value (the legacy default stream)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_switch = nullptr;            // orders work across ecgpu_set_stream
  char err[512] = {0};
  std::mutex mu;
  std::mutex err_mu;                          // guards err[] (ecgpu_set_err / ecgpu_last_error_copy)
  int64_t opt[ECGPU_OPT_COUNT_] = {0, 26, 0, 0, 1, 0, 4, 0, 0, 0, 0, (int64_t)1 << 31, 0};      // ecgpu_option defaults
  // grow-only device staging buffers for ECGPU_MEM_HOST calls: 6 for whole-batch staging, then PIPE_NSLOT pipeline slots x PIPE_ARGS0 arguments.
  // The message-level signing calls have a seventh buffer (four inputs): its slots follow behind, so that every older slot keeps its
  // number - STAGE_IN3 for a whole batch, then one per pipeline slot (hostpipe::stage_index).
  static constexpr int PIPE_NSLOT = 3, PIPE_ARGS0 = 6, PIPE_MAXARGS = 7, PIPE_STAGE0 = 6;
  static constexpr int STAGE_IN3 = PIPE_STAGE0 + PIPE_NSLOT * PIPE_ARGS0, PIPE_STAGE1 = STAGE_IN3 + 1;
  static constexpr int NSTAGE = PIPE_STAGE1 + PIPE_NSLOT * (PIPE_MAXARGS - PIPE_ARGS0);
  DevBuf stage[NSTAGE];
  // chunked host-buffer pipeline (host_pipe.hpp): download and upload streams, per-slot events (inputs arrived / kernels done /
  // outputs read), and the page-locked bounce buffers pageable caller memory is copied through ([0] uploads, [1] downloads)
  static constexpr int PIPE_NWORK = 4;
  static constexpr size_t PIPE_BOUNCE = (size_t)4 << 20;
  hipStream_t copy_stream = nullptr;
  hipStream_t up_stream = nullptr;
  hipEvent_t ev_kernel[PIPE_NSLOT] = {};
  hipEvent_t ev_up[PIPE_NSLOT] = {};
  hipEvent_t ev_down[PIPE_NSLOT] = {};
  void* bounce[2][PIPE_NWORK] = {};
  hipEvent_t ev_bounce[2][PIPE_NWORK] = {};
  void* table[ECGPU_TAB_COUNT_][3] = {};             // [kind][curve]
  size_t fb_bytes[3] = {0, 0, 0};                      // device memory held by the generator tables of a curve
  int fb_widest[3] = {0, 0, 0};
  // Tables of shared points (ECGPU_SHARED_POINTS; ecgpu.hip, shared points): keyed by curve, the point's affine bytes and the window
  // width, at most SHARED_TABLES_PER_CURVE per curve and ECGPU_OPT_SHARED_TABLE_BUDGET bytes over all, least recently used out first.
  // An allocation holds the table and, behind it, the point's canonical x || y words (what a shared key's prep kernel reads).
  struct SharedTable {
    void* p;
    size_t bytes;              // of the table itself; the point's words follow
    int curve, wb;
    uint64_t used;             // shared_clock at the last call that used it
    uint8_t key[96];           // x || y, 2 NB bytes
  };
  static constexpr size_t SHARED_TABLES_PER_CURVE = 16;
  std::vector<SharedTable> shared_tabs;
  uint64_t shared_clock = 0;
  size_t shared_bytes = 0;
  // the call's points on the device, their validation flags, the builders' window bases and the broadcast path's replicated points
  DevBuf shared_ws;
  // Workspaces (grow-only; DESIGN section 1, Workspaces).  The rule: the OUTERMOST launcher of a call carves a buffer, once
  // (ecgpu_carve below); whatever it calls receives pointers and never carves that buffer again - growing loses the contents.
  // per-lane tables of the variable-base, Straus and reference kernels: one buffer used whole, reserved by the launcher of that kernel
  DevBuf tab_ws;
  // MSM workspace: carved by msm_run / msm_buckets (msm_kernels.hpp)
  DevBuf msm_ws;
  // work counters of the dynamically scheduled kernels (sched.hpp): a small ring, one 8-byte counter per launch, zeroed on the stream before it
  unsigned long long* sched_ctr = nullptr;
  unsigned sched_next = 0;
  // intermediates of the pipelines: carved by the curve's entry launcher (curve_ops.hpp), or by the API layer (ecgpu.hip) where
  // the launchers it strings together carve nothing
  DevBuf ecdsa_ws;
  // BIP340 challenges of ecgpu_schnorr_verify_prehash_batch and the digests of the message-level calls (with the challenges or the
  // zero aux_rand behind them: one carve), carved by the API layer: they live through the prehash launchers, which carve ecdsa_ws
  DevBuf hash_ws;
};

static inline int ecgpu_set_err(ecgpu_ctx* c, int code, const char* fmt, ...) {
  if (c) {
    std::lock_guard<std::mutex> lk(c->err_mu);
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c->err, sizeof(c->err), fmt, ap);
    va_end(ap);
  }
  return code;
}
#define HIPCHK(c, call)                                                                                        \
  do {                                                                                                         \
    hipError_t e_ = (call);                                                                                    \
    if (e_ != hipSuccess) return ecgpu_set_err(c, ECGPU_ERR_RUNTIME, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)

// Makes `b` hold at least `need` bytes.  Growing waits for the work queued on the old buffer, frees it and allocates anew: the
// contents are lost and the new memory is not cleared.
static inline int ecgpu_reserve(ecgpu_ctx* c, DevBuf& b, size_t need) {
  if (need <= b.cap) return 0;
  if (b.p) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(b.p));
  }
  b.p = nullptr;
  b.cap = 0;
  HIPCHK(c, hipMalloc(&b.p, need));
  b.cap = need;
  return 0;
}
// Carves `b` into the sub-buffers `layout` asks for (ws_carver.hpp): runs it once to add the sizes up, reserves, runs it again
// to hand out the pointers.
template <class Layout>
static inline int ecgpu_carve(ecgpu_ctx* c, DevBuf& b, Layout&& layout) {
  WsCarver sizes{nullptr};
  layout(sizes);
  int rc = ecgpu_reserve(c, b, sizes.total);
  if (rc) return rc;
  WsCarver ws{(char*)b.p};
  layout(ws);
  return 0;
}

// the counter of the next dynamically scheduled launch (sched.hpp), zeroed on the context's stream; nullptr on failure (error text set)
static inline unsigned long long* ecgpu_sched_counter(ecgpu_ctx* c) {
  constexpr unsigned RING = 64;
  if (!c->sched_ctr) {
    if (hipMalloc((void**)&c->sched_ctr, RING * sizeof(unsigned long long)) != hipSuccess) { ecgpu_set_err(c, ECGPU_ERR_RUNTIME, "hipMalloc of the work counters failed"); return nullptr; }
  }
  unsigned long long* p = c->sched_ctr + (c->sched_next++ % RING);
  if (hipMemsetAsync(p, 0, sizeof(unsigned long long), c->stream) != hipSuccess) { ecgpu_set_err(c, ECGPU_ERR_RUNTIME, "hipMemsetAsync of a work counter failed"); return nullptr; }
  return p;
}
// Clears b bytes at p on the context's stream when the scope ends, whichever way a launcher is left: for secrets that pass through a workspace
struct StreamWipe {
  ecgpu_ctx* c; void* p; size_t b;
  ~StreamWipe() { (void)hipMemsetAsync(p, 0, b, c->stream); }
};
static inline unsigned ecgpu_grid_for(const ecgpu_ctx* c, size_t n, int per_cu) {
  size_t blocks = (n + 255) / 256;
  size_t cap = (size_t)c->num_cus * per_cu;
  if (blocks > cap) blocks = cap;
  if (blocks == 0) blocks = 1;
  return (unsigned)blocks;
}

// Grid of a kernel with STATIC work (lane t takes units t, t + T, ...) and one inversion per `batch` results of a lane: up to `max_mult` times the
// resident workgroups, as far as every lane keeps a full batch.  Waves that share a SIMD do not progress evenly, so a grid of exactly the resident
// workgroups ends ragged (work distribution); more, shorter workgroups fill the gaps and the choice depends on the batch size only
// (constant-time kernels cannot draw work dynamically).  Signing, 2^22 per call: 17.6 -> 16.4 ms (k256), 19.0 -> 18.0 ms (P-256); at 2^20, where a lane
// has four results, oversubscribing would halve the inversion's amortisation and loses 1-4 %: the rule leaves that size alone.
static inline unsigned ecgpu_grid_oversubscribed(const ecgpu_ctx* c, size_t n, int per_cu, int batch, int max_mult) {
  const size_t resident = (size_t)c->num_cus * per_cu;
  size_t mult = n / (resident * 256 * (size_t)batch);
  if (mult < 1) mult = 1;
  if (mult > (size_t)max_mult) mult = max_mult;
  size_t blocks = (n + 255) / 256;
  if (blocks > resident * mult) blocks = resident * mult;
  if (blocks == 0) blocks = 1;
  return (unsigned)blocks;
}

// Kernel launchers of one curve; all pointers are device pointers, everything is asynchronous on c->stream.
struct ecgpu_curve_ops {
  int (*field_op)(ecgpu_ctx* c, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n);
  int (*point_op)(ecgpu_ctx* c, int op, const uint32_t* p, const uint32_t* q, uint32_t* out, size_t n);
  int (*point_eq)(ecgpu_ctx* c, const uint32_t* p, const uint32_t* q, uint8_t* eq, size_t n);
  int (*normalize)(ecgpu_ctx* c, const uint32_t* p, uint32_t* out_xy, uint8_t* out_inf, size_t n);
  int (*lincomb)(ecgpu_ctx* c, const uint32_t* scalars, const uint32_t* points, int pt_fmt, size_t terms, uint32_t* out,
                 int out_fmt, uint8_t* out_inf, size_t n, unsigned flags);
  int (*msm)(ecgpu_ctx* c, const uint32_t* scalars, const uint32_t* points, int pt_fmt, size_t n, uint32_t* out, int out_fmt);
  int (*validate_scalars)(ecgpu_ctx* c, const uint32_t* scalars, uint8_t* ok, size_t n, size_t terms);
  int (*validate_points)(ecgpu_ctx* c, const uint32_t* xy, uint8_t* ok, size_t n);
  int (*decompress)(ecgpu_ctx* c, const uint32_t* x, const uint8_t* y_is_odd, uint32_t* out_xy, uint8_t* ok, size_t n);
  int (*synth_scalars)(ecgpu_ctx* c, uint64_t seed, uint64_t first, uint32_t* out, size_t n);
  int (*synth_points)(ecgpu_ctx* c, uint64_t seed, uint64_t first, uint32_t* out_xy, size_t n);
  int (*to_bytes)(ecgpu_ctx* c, const uint32_t* pts, int pt_fmt, uint8_t* out, size_t n);
  int (*from_bytes)(ecgpu_ctx* c, const uint8_t* in, uint32_t* out_xy, uint8_t* ok, size_t n);
  int (*sec1_encode)(ecgpu_ctx* c, const uint32_t* pts, int pt_fmt, int compress, uint8_t* out, size_t n);
  int (*sec1_decode)(ecgpu_ctx* c, const uint8_t* in, size_t record_bytes, uint32_t* out_xy, uint8_t* ok, size_t n);
  int (*ecdsa_verify)(ecgpu_ctx* c, const uint32_t* z, const uint32_t* sig, const uint32_t* q_xy, uint8_t* ok, size_t n, unsigned flags);
  int (*h2c_map)(ecgpu_ctx* c, const uint32_t* u, int count, uint32_t* out_xy, uint8_t* out_inf, size_t n);
  int (*ecdsa_recover)(ecgpu_ctx* c, const uint32_t* z, const uint32_t* sig, const uint8_t* recid, uint32_t* out_xy, uint8_t* ok, size_t n,
                       unsigned flags);
  int (*schnorr_verify)(ecgpu_ctx* c, const uint32_t* px, const uint32_t* sig, const uint32_t* e, uint8_t* ok, size_t n);
  int (*ecdsa_sign)(ecgpu_ctx* c, const uint32_t* d, const uint32_t* k, const uint32_t* z, uint32_t* sig, uint8_t* recid, uint8_t* ok,
                    size_t n, unsigned flags);
  int (*ecdh)(ecgpu_ctx* c, const uint32_t* d, const uint32_t* q_xy, uint32_t* shared_x, uint8_t* ok, size_t n);
  // units of one whole pass of the kernel `lincomb` would pick: every resident lane gets its full sub-batch (the results that share
  // one inversion).  The host-buffer pipeline sizes its chunks by it (host_pipe.hpp).
  size_t (*pass_units)(const ecgpu_ctx* c, int has_points, size_t terms, unsigned flags);
  // scalar field (scalar_ops.hpp): canonical big-endian scalars in and out; ok may be NULL
  int (*scalar_op)(ecgpu_ctx* c, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint8_t* ok, size_t n);
  int (*scalar_reduce)(ecgpu_ctx* c, const uint8_t* in, size_t in_bytes, uint32_t* out, size_t n, unsigned flags);
  // hash layer (h2c_hash.hpp).  h2c_hash_to_field: expand_message_xmd on the curve's hash fused with FromOkm, u = n x count field
  // elements as h2c_map reads them (msg_len may be NULL; tail.out_len = count L); field_from_okm: n records of L bytes -> n field
  // elements; schnorr_challenge: e = n BIP340 challenge hashes (secp256k1 only)
  int (*h2c_hash_to_field)(ecgpu_ctx* c, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, const ecgpu::h2c::XmdTail& tail, int count,
                           uint32_t* u, size_t n);
  int (*field_from_okm)(ecgpu_ctx* c, const uint8_t* okm, uint32_t* out, size_t n);
  int (*schnorr_challenge)(ecgpu_ctx* c, const uint32_t* px, const uint32_t* sig, const uint32_t* prehash, uint32_t* e, size_t n);
  // deterministic signing (signing_kernels.hpp).  rfc6979_nonce: k = n RFC 6979 nonces (extra may be NULL), 0 for a key out of range;
  // ecdsa_sign_prehash: the nonces go through the workspace into ecdsa_sign and are cleared; schnorr_sign_prehash: BIP340
  // sign_prehash_with_aux_rand (secp256k1 only; pubkeys_x may be NULL)
  int (*rfc6979_nonce)(ecgpu_ctx* c, const uint32_t* d, const uint32_t* z, const uint32_t* extra, uint32_t* k, size_t n);
  int (*ecdsa_sign_prehash)(ecgpu_ctx* c, const uint32_t* d, const uint32_t* z, const uint32_t* extra, uint32_t* sig, uint8_t* recid, uint8_t* ok,
                            size_t n, unsigned flags);
  int (*schnorr_sign_prehash)(ecgpu_ctx* c, const uint32_t* d, const uint32_t* m, const uint32_t* aux, uint32_t* sig, uint32_t* pubkeys_x, uint8_t* ok,
                              size_t n);
  // BIP340 batch verification (schnorr_batch_kernels.hpp; secp256k1 only): ONE equation over the n signatures, whose coefficients are those
  // of elements first_index .. of the caller's batch under seed32 (32 bytes of HOST memory).  Synchronises the stream; *verdict = every
  // element valid.  ok (NULL allowed with ECGPU_BATCH_VERDICT_ONLY) as include/ecgpu.h describes.
  int (*schnorr_batch_verify)(ecgpu_ctx* c, const uint32_t* px, const uint32_t* sig, const uint32_t* e, uint8_t* ok, size_t n, uint64_t first_index,
                              const uint8_t* seed32, unsigned flags, int* verdict);
  // shared points (sharedbase.hpp; the cache of the tables is the API layer's, ecgpu.hip).  shared_table_bytes: size of a table of
  // window width wb (5 | 8 | 16 | 20), 0 for any other width; shared_build: enqueues the two builder stages for the point at xy (device
  // memory, canonical words; `bases` is scratch for one entry per window); shared_lincomb: out[i] = sum_t sc[i terms + t] H_t from
  // `terms` <= 8 tables of width wb (a null table: the identity; ECGPU_SECRET_SCALARS: one table of width 5 on the constant-time
  // kernel); broadcast_points: dst = the `terms` points at xy repeated n times; ecdsa_verify_shared: ecdsa_verify whose u2 Q runs on
  // Q's table, q_rep holding Q repeated n times for the prep kernel
  size_t (*shared_table_bytes)(int wb);
  int (*shared_build)(ecgpu_ctx* c, const uint32_t* xy, int wb, void* bases, void* table);
  int (*shared_lincomb)(ecgpu_ctx* c, const uint32_t* sc, const void* const* tables, int wb, size_t terms, uint32_t* out, int out_fmt, uint8_t* out_inf,
                        size_t n, unsigned flags);
  int (*broadcast_points)(ecgpu_ctx* c, const uint32_t* xy, size_t terms, uint32_t* dst, size_t n);
  int (*ecdsa_verify_shared)(ecgpu_ctx* c, const uint32_t* z, const uint32_t* sig, const uint32_t* q_rep, const void* table, int wb, uint8_t* ok, size_t n,
                             unsigned flags);
};
// Signatures from which ecgpu_schnorr_batch_verify* takes the equation by default.  Under the MSM's small-sum limit (2n + 1 below
// msm_kernels.hpp SMALL_MSM_TERMS; msm_k256.hip asserts the relation) the MSM is itself one multiplication per term and the equation
// cannot win; measured, device-resident, equation against per-signature call (profiles/schnorr_batch_verify.txt): 2^16 1.71 / 1.73 ms
// (inside the spread of the runs), 2^18 2.71 / 3.68 ms, 2^20 6.08 / 10.8 ms, 2^22 19.2 / 35.5 ms - 2^18 is the smallest measured size at
// which it wins.
constexpr size_t ECGPU_SCHNORR_BATCH_MIN = (size_t)1 << 18;
// expand_message_xmd to raw bytes on `hash` (ecgpu_hash), curve-independent (h2c_hash.hip): out = n x tail.out_len bytes
int ecgpuint_xmd(ecgpu_ctx* c, int hash, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, const ecgpu::h2c::XmdTail& tail, uint8_t* out, size_t n);
// plain digests on `hash` (h2c_hash.hip): out = n rows of 32 / 48 bytes, 4-byte aligned
int ecgpuint_digest(ecgpu_ctx* c, int hash, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, uint32_t* out, size_t n);
// the sponge ids of ecgpuint_digest (keccak.hip): Keccak-256, SHA3-256, SHA3-384; any other id is refused
int ecgpuint_keccak_digest(ecgpu_ctx* c, int hash, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, uint32_t* out, size_t n);
// Pippenger MSM, one translation unit per curve (msm_*.hip); `mul` is the curve's batch scalar multiplication (affine in / out
// on device memory), used for small sums
typedef int (*ecgpu_msm_mul_fn)(ecgpu_ctx* c, const uint32_t* scalars, const uint32_t* points, int pt_fmt, uint32_t* out_xy, size_t n);
int ecgpu_msm_k256(ecgpu_ctx* c, const uint32_t* sc, const uint32_t* pts, int pt_fmt, size_t n, uint32_t* out, int out_fmt, ecgpu_msm_mul_fn mul);
int ecgpu_msm_p256(ecgpu_ctx* c, const uint32_t* sc, const uint32_t* pts, int pt_fmt, size_t n, uint32_t* out, int out_fmt, ecgpu_msm_mul_fn mul);
int ecgpu_msm_p384(ecgpu_ctx* c, const uint32_t* sc, const uint32_t* pts, int pt_fmt, size_t n, uint32_t* out, int out_fmt, ecgpu_msm_mul_fn mul);
const ecgpu_curve_ops* ecgpu_ops_k256();
const ecgpu_curve_ops* ecgpu_ops_p256();
const ecgpu_curve_ops* ecgpu_ops_p384();
// ecgpu_msm with the inputs and the result in different kinds of memory (ecgpu.hip; used by the device group, group.hip)
int ecgpuint_msm_mixed(ecgpu_ctx* c, int curve, const uint8_t* scalars, const uint8_t* points, int pt_fmt, size_t n, uint8_t* out, int out_fmt,
                       int mem_in, int mem_out);
// secp256k1 kernels that run on SECRET scalars live in their own translation unit (ops_k256_ct.hip), compiled with
// ECGPU_K256_BRANCHFREE: the field additions / subtractions / folds there ripple their rare carries unconditionally, so no branch
// depends on data.  These launchers are what the generic code (curve_ops.hpp) calls for curve 0.
int ecgpuint_k256_mul_ct(ecgpu_ctx* c, const uint32_t* sc, const uint32_t* pts, int pt_fmt, uint32_t* out, int out_fmt, uint8_t* out_inf, size_t n);        // k P, varbase_ct_k256.hpp
int ecgpuint_k256_mul_gen_ct(ecgpu_ctx* c, const uint32_t* sc, const void* table, uint32_t* out, int out_fmt, uint8_t* out_inf, size_t n);                 // k G, fixedbase_ct.hpp
// the reference schedules (exact X, Y, Z; constant-time table scans): points == NULL is mul_by_generator over `gen_table`
int ecgpuint_k256_reference(ecgpu_ctx* c, const uint32_t* sc, const uint32_t* pts, int pt_fmt, size_t terms, const void* gen_table, uint32_t* out, int out_fmt,
                            uint8_t* out_inf, size_t n);
size_t ecgpuint_k256_ct_pass_units(const ecgpu_ctx* c);
