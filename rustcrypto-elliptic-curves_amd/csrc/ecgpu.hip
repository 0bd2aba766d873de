// C ABI of libecgpu.so (include/ecgpu.h): context, staging of host buffers, dispatch to the
// per-curve kernel launchers (ops_*.hip).  Host side of the boundary; all arithmetic happens in
// the gfx950 kernels.  There is deliberately no CPU code path in this library.
//
// Every batched entry point is three parts: its argument checks, ONE list of its caller buffers (CallArg: pointer, direction,
// bytes per element, secret or not) and one launch lambda, the only place that casts to the launcher's pointer types.
// run_batch does the rest from the list.  Device memory: the pointers pass through.  Host memory: the buffers are staged in the
// context's grow-only device slots - whole, the i-th input of the list in slot {0, 1, 4, 24}[i] and the j-th output in {2, 3, 5}[j]
// (an absent optional buffer keeps its place in the count), or, for the calls that name a pass size and from PIPE_MIN elements
// on, in chunks through the pipeline (host_pipe.hpp), list entry a of pipeline slot s in slot 6 + 6 s + a (a seventh entry: 25 + s).  What the list marks
// secret is cleared from its slots (and from the pipeline's bounce buffers) before the call returns, whichever way it ends.
#include <errno.h>
#include <string.h>
#include <sys/random.h>
#include <condition_variable>
#include <thread>
#include <vector>

#include "ecgpu_internal.hpp"
#include "host_pipe.hpp"

static int stage_reserve(ecgpu_ctx* c, int slot, size_t bytes) {
  DevBuf& b = c->stage[slot];
  if (bytes <= b.cap) return 0;
  int rc = ecgpu_reserve(c, b, bytes + bytes / 4 + 256);
  if (rc) return rc;
  // recycled memory keeps its old contents: a slot starts out zero, its slack included (waited for: the pipeline's own streams use it next)
  HIPCHK(c, hipMemsetAsync(b.p, 0, b.cap, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// The device view of one caller buffer: the pointer itself, or staging slot `slot` (an input is copied into it).
static int stage_arg(ecgpu_ctx* c, int slot, const void* p, size_t bytes, bool is_out, int mem, void** dev) {
  *dev = nullptr;
  if (!p || bytes == 0) return 0;
  if (mem == ECGPU_MEM_DEVICE) { *dev = const_cast<void*>(p); return 0; }
  int rc = stage_reserve(c, slot, bytes);
  if (rc) return rc;
  *dev = c->stage[slot].p;
  if (!is_out) HIPCHK(c, hipMemcpyAsync(*dev, p, bytes, hipMemcpyHostToDevice, c->stream));
  return 0;
}
// a staged output goes back to the caller's buffer
static int unstage_out(ecgpu_ctx* c, void* p, const void* dev, size_t bytes, int mem) {
  if (dev && mem != ECGPU_MEM_DEVICE) HIPCHK(c, hipMemcpyAsync(p, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  return 0;
}
static int finish_host(ecgpu_ctx* c, int mem) {
  if (mem == ECGPU_MEM_HOST) HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Host-buffer calls on large batches stream through the device in chunks (host_pipe.hpp): batches of PIPE_MIN units and more.
// `pass` is the number of units that gives every resident lane of the dominant kernel its full sub-batch (the curve's
// ops->pass_units): chunks grow from pass / 8 to pass and the last one is small again.
// ---------------------------------------------------------------------------------------------
static constexpr size_t PIPE_MIN = (size_t)1 << 21;
// one multi-scalar multiplication from host memory: sums of MSM_PIPE_MIN terms and more are cut into parts of MSM_PIPE_PART terms
// (a part is one slab of either window width: msm_kernels.hpp Geo<CB>::SLAB_TERMS >= 2^23)
static constexpr size_t MSM_PIPE_MIN = (size_t)1 << 22, MSM_PIPE_PART = (size_t)1 << 23;
extern "C" int ecgpu_host_chunk_schedule(size_t n, size_t pass_units, size_t* sizes, size_t cap);

// One caller buffer of a batched call.
struct CallArg {
  const void* ptr;     // host or device memory, as the call's `mem` says
  bool is_out;
  size_t unit;         // bytes per batch element
  bool secret;         // its staged copy does not outlive the call
  bool optional;       // NULL means absent
};
enum : unsigned { ARG_SECRET = 1, ARG_OPTIONAL = 2 };
static constexpr CallArg arg_in(const void* p, size_t unit, unsigned flags = 0) { return {p, false, unit, (flags & ARG_SECRET) != 0, (flags & ARG_OPTIONAL) != 0}; }
static constexpr CallArg arg_out(void* p, size_t unit, unsigned flags = 0) { return {p, true, unit, (flags & ARG_SECRET) != 0, (flags & ARG_OPTIONAL) != 0}; }

// The slot rule (include/ecgpu.h, ecgpu_debug_workspace).  Staged whole, list entry k goes by its direction and by how many
// entries of that direction precede it, present or absent; in the pipeline by its position alone (hostpipe::stage_index).
static constexpr int WHOLE_IN_SLOT[4] = {0, 1, 4, ecgpu_ctx::STAGE_IN3}, WHOLE_OUT_SLOT[3] = {2, 3, 5};
static constexpr int whole_slot(const CallArg* args, int k) {
  int before = 0;
  for (int i = 0; i < k; i++) before += args[i].is_out == args[k].is_out;
  return (args[k].is_out ? WHOLE_OUT_SLOT : WHOLE_IN_SLOT)[before];
}
namespace slot_rule_check {
// the shape of ecgpu_ecdsa_sign_batch, the longest list: d, k, z in; sig, recid, ok out
constexpr CallArg sign[6] = {arg_in(nullptr, 32), arg_in(nullptr, 32), arg_in(nullptr, 32), arg_out(nullptr, 64), arg_out(nullptr, 1), arg_out(nullptr, 1)};
static_assert(whole_slot(sign, 0) == 0 && whole_slot(sign, 1) == 1 && whole_slot(sign, 2) == 4, "inputs of a whole batch: slots 0, 1, 4");
static_assert(whole_slot(sign, 3) == 2 && whole_slot(sign, 4) == 3 && whole_slot(sign, 5) == 5, "outputs of a whole batch: slots 2, 3, 5");
// ecgpu_ecdsa_recover_batch: z, sig, recid in; keys, ok out
constexpr CallArg recover[5] = {arg_in(nullptr, 32), arg_in(nullptr, 64), arg_in(nullptr, 1), arg_out(nullptr, 64), arg_out(nullptr, 1)};
static_assert(whole_slot(recover, 2) == 4 && whole_slot(recover, 3) == 2 && whole_slot(recover, 4) == 3, "recover: recovery ids in 4, keys in 2, ok in 3");
static_assert(ecgpu_ctx::PIPE_STAGE0 == 6 && ecgpu_ctx::PIPE_ARGS0 == 6 && ecgpu_ctx::PIPE_NSLOT == 3, "6 whole-batch slots, then 3 pipeline slots of 6 arguments");
// ecgpu_ecdsa_sign_msg_batch, seven buffers: d, msgs, msg_len, extra in; sig, recid, ok out
constexpr CallArg sign_msg[7] = {arg_in(nullptr, 32), arg_in(nullptr, 1), arg_in(nullptr, 4), arg_in(nullptr, 32), arg_out(nullptr, 64), arg_out(nullptr, 1), arg_out(nullptr, 1)};
static_assert(whole_slot(sign_msg, 3) == 24 && whole_slot(sign_msg, 4) == 2 && whole_slot(sign_msg, 6) == 5, "a fourth input: slot 24; the outputs keep 2, 3, 5");
static_assert(hostpipe::stage_index(0, 6) == 25 && hostpipe::stage_index(2, 6) == 27, "a seventh argument of pipeline slot s: 25 + s");
static_assert(hostpipe::stage_index(0, 0) == 6 && hostpipe::stage_index(1, 2) == 14 && hostpipe::stage_index(2, 5) == 23, "argument a of pipeline slot s: 6 + 6 s + a");
static_assert(hostpipe::stage_index(ecgpu_ctx::PIPE_NSLOT - 1, ecgpu_ctx::PIPE_MAXARGS - 1) == ecgpu_ctx::NSTAGE - 1 && ecgpu_ctx::NSTAGE == 28, "the last staging slot");
}  // namespace slot_rule_check

// Staged copies of secret scalars do not outlive the call (the reference zeroizes its secrets): the guard clears the
// bytes this call staged in its slots on EVERY exit path, the error returns included, and waits for the clearing.
struct SecretWipe {
  ecgpu_ctx* c;
  static constexpr int CAP = 3 * ecgpu_ctx::PIPE_NSLOT + 3;      // no call marks more than three of its buffers secret
  int slot[CAP];
  size_t bytes[CAP];
  int cnt = 0;
  explicit SecretWipe(ecgpu_ctx* ctx) : c(ctx) {}
  void arm(int s, size_t b) { if (cnt < CAP) { slot[cnt] = s; bytes[cnt] = b; cnt++; } }
  // argument `a` of every pipeline slot, whole capacity (the chunk sizes vary)
  void arm_pipeline(int a) { for (int sl = 0; sl < ecgpu_ctx::PIPE_NSLOT; sl++) arm(hostpipe::stage_index(sl, a), (size_t)-1); }
  ~SecretWipe() {
    if (!cnt) return;
    for (int i = 0; i < cnt; i++) {
      const DevBuf& s = c->stage[slot[i]];
      const size_t b = bytes[i] < s.cap ? bytes[i] : s.cap;
      if (s.p && b) (void)hipMemsetAsync(s.p, 0, b, c->stream);
    }
    (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
  }
};

// One batched call over the buffers of `args`: launch(dev, cnt) enqueues the kernels for cnt elements on c->stream, dev[k] being
// the device view of args[k] (nullptr for an absent one).  pass_units is the curve's ops->pass_units for the call's dominant
// kernel; 0: the call never streams in chunks.
template <size_t N, class Launch>
static int run_batch(ecgpu_ctx* c, int mem, size_t n, const CallArg (&args)[N], size_t pass_units, Launch launch) {
  static_assert(N <= (size_t)ecgpu_ctx::PIPE_MAXARGS, "a pipeline slot stages PIPE_MAXARGS arguments");
  for (const CallArg& a : args)
    if (!a.ptr && !a.optional) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  const bool host = mem == ECGPU_MEM_HOST;
  SecretWipe wipe(c);
  if (host && pass_units && n >= PIPE_MIN) {
    hostpipe::Arg pa[N];
    bool secret = false;
    for (size_t k = 0; k < N; k++) {
      pa[k] = {args[k].is_out ? nullptr : args[k].ptr, args[k].is_out ? const_cast<void*>(args[k].ptr) : nullptr, args[k].unit};
      if (args[k].secret) { wipe.arm_pipeline((int)k); secret = true; }
    }
    std::vector<size_t> sizes((size_t)ecgpu_host_chunk_schedule(n, pass_units, nullptr, 0));
    (void)ecgpu_host_chunk_schedule(n, pass_units, sizes.data(), sizes.size());
    return hostpipe::run(c, pa, (int)N, sizes, secret, [&](int slot, size_t bytes) { return stage_reserve(c, slot, bytes); },
                         [&](void** d, size_t cnt, size_t) { return launch(d, cnt); });
  }
  if (host)
    for (size_t k = 0; k < N; k++)
      if (args[k].secret) wipe.arm(whole_slot(args, (int)k), n * args[k].unit);
  void* dev[N];
  int rc;
  for (size_t k = 0; k < N; k++)
    if ((rc = stage_arg(c, whole_slot(args, (int)k), args[k].ptr, n * args[k].unit, args[k].is_out, mem, &dev[k]))) return rc;
  if ((rc = launch(dev, n))) return rc;
  for (size_t k = 0; k < N; k++)
    if (args[k].is_out && (rc = unstage_out(c, const_cast<void*>(args[k].ptr), dev[k], n * args[k].unit, mem))) return rc;
  return finish_host(c, mem);
}

static const ecgpu_curve_ops* ops_for(int curve) {
  switch (curve) {
    case ECGPU_K256: return ecgpu_ops_k256();
    case ECGPU_P256: return ecgpu_ops_p256();
    case ECGPU_P384: return ecgpu_ops_p384();
    default: return nullptr;
  }
}
#define ENTER(c, curve)                                                                              \
  const ecgpu_curve_ops* ops = ops_for(curve);                                                       \
  if (!ops) return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "curve %d not supported", curve);         \
  std::lock_guard<std::mutex> lk(c->mu);                                                             \
  HIPCHK(c, hipSetDevice(c->device));                                                                \
  const size_t nb = ecgpu_field_bytes(curve);                                                        \
  (void)nb

extern "C" {

const char* ecgpu_version(void) { return "ecgpu 0.11 (gfx950)"; }

size_t ecgpu_field_bytes(int curve) {
  switch (curve) {
    case ECGPU_K256: return 32;
    case ECGPU_P256: return 32;
    case ECGPU_P384: return 48;
    default: return 0;
  }
}
size_t ecgpu_hash_bytes(int hash) {
  switch (hash) {
    case ECGPU_SHA256: case ECGPU_KECCAK256: case ECGPU_SHA3_256: return 32;
    case ECGPU_SHA384: case ECGPU_SHA3_384: return 48;
    default: return 0;
  }
}

int ecgpu_create(ecgpu_ctx** out, int device_index) {
  if (!out) return ECGPU_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ECGPU_ERR_NO_DEVICE;
  if (device_index < 0 || device_index >= ndev) return ECGPU_ERR_ARG;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_index) != hipSuccess) return ECGPU_ERR_NO_DEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return ECGPU_ERR_NO_DEVICE;   // kernels exist for gfx950 only
  ecgpu_ctx* c = new ecgpu_ctx();
  c->device = device_index;
  c->num_cus = prop.multiProcessorCount;
  if (hipSetDevice(device_index) != hipSuccess || hipStreamCreateWithFlags(&c->own_stream, hipStreamDefault) != hipSuccess ||
      hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_switch, hipEventDisableTiming) != hipSuccess) {
    delete c;
    return ECGPU_ERR_RUNTIME;
  }
  c->stream = c->own_stream;
  *out = c;
  return ECGPU_OK;
}

void ecgpu_destroy(ecgpu_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (int i = 0; i < ecgpu_ctx::NSTAGE; i++)
    if (c->stage[i].p) {                     // staging slots may have held secret scalars: clear before release
      (void)hipMemset(c->stage[i].p, 0, c->stage[i].cap);
      (void)hipFree(c->stage[i].p);
    }
  for (int i = 0; i < ecgpu_ctx::PIPE_NSLOT; i++) {
    if (c->ev_kernel[i]) (void)hipEventDestroy(c->ev_kernel[i]);
    if (c->ev_up[i]) (void)hipEventDestroy(c->ev_up[i]);
    if (c->ev_down[i]) (void)hipEventDestroy(c->ev_down[i]);
  }
  for (int d = 0; d < 2; d++)
    for (int w = 0; w < ecgpu_ctx::PIPE_NWORK; w++) {
      if (c->bounce[d][w]) { memset(c->bounce[d][w], 0, ecgpu_ctx::PIPE_BOUNCE); (void)hipHostFree(c->bounce[d][w]); }
      if (c->ev_bounce[d][w]) (void)hipEventDestroy(c->ev_bounce[d][w]);
    }
  if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
  if (c->up_stream) (void)hipStreamDestroy(c->up_stream);
  for (auto& kind : c->table)
    for (void* t : kind)
      if (t) (void)hipFree(t);
  for (const ecgpu_ctx::SharedTable& t : c->shared_tabs) (void)hipFree(t.p);
  for (DevBuf* b : {&c->msm_ws, &c->tab_ws, &c->ecdsa_ws, &c->hash_ws, &c->shared_ws})
    if (b->p) (void)hipFree(b->p);
  if (c->sched_ctr) (void)hipFree(c->sched_ctr);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->ev_switch) (void)hipEventDestroy(c->ev_switch);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

// The per-context scratch (staging slots, table / MSM / ECDSA workspaces, lazily built tables) is shared by
// consecutive calls, so work queued on the old stream must be ordered before anything the new stream does:
// an event recorded on the old stream is waited for by the new one.  If the old stream cannot take the record any
// more (the caller destroyed it), a device-wide synchronisation gives the same ordering; the new stream is installed
// either way, so a context never stays pinned to a dead stream.
static int switch_stream(ecgpu_ctx* c, hipStream_t next) {
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  if (next == c->stream) return ECGPU_OK;
  hipError_t e = hipEventRecord(c->ev_switch, c->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(next, c->ev_switch, 0);
  if (e != hipSuccess) {
    (void)hipGetLastError();                  // not sticky: the next launch check must not report it
    (void)hipDeviceSynchronize();
  }
  c->stream = next;
  return ECGPU_OK;
}
// NULL is the legacy default stream, as for every HIP API (PyTorch's default stream has this handle)
int ecgpu_set_stream(ecgpu_ctx* c, void* s) {
  if (!c) return ECGPU_ERR_ARG;
  return switch_stream(c, (hipStream_t)s);
}
int ecgpu_use_own_stream(ecgpu_ctx* c) {
  if (!c) return ECGPU_ERR_ARG;
  return switch_stream(c, c->own_stream);
}
int ecgpu_synchronize(ecgpu_ctx* c) {
  if (!c) return ECGPU_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ECGPU_OK;
}
const char* ecgpu_last_error(const ecgpu_ctx* c) { return c ? c->err : "null context"; }
int ecgpu_last_error_copy(ecgpu_ctx* c, char* buf, size_t cap) {
  if (!c || !buf || cap == 0) return ECGPU_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->err_mu);
  strncpy(buf, c->err, cap - 1);
  buf[cap - 1] = 0;
  return ECGPU_OK;
}

int ecgpu_set_option(ecgpu_ctx* c, int option, int64_t v) {
  if (!c) return ECGPU_ERR_ARG;
  bool ok = false;
  switch (option) {
    case ECGPU_OPT_FB_WINDOW: ok = (v == 0 || v == 8 || v == 16 || v == 20 || v == 24 || v == 26); break;
    case ECGPU_OPT_FB_MAX_WINDOW: ok = (v == 8 || v == 16 || v == 20 || v == 24 || v == 26); break;
    case ECGPU_OPT_MSM_WINDOW_BITS: ok = (v == 0 || v == 16 || v == 19); break;
    case ECGPU_OPT_MSM_SLAB_TERMS: ok = (v == 0 || (v >= 1024 && v <= ((int64_t)1 << 24))); break;
    case ECGPU_OPT_MSM_SMALL_PATH: ok = (v == 0 || v == 1); break;
    case ECGPU_OPT_MSM_ROUNDS: ok = (v >= 0 && v <= 64); break;
    case ECGPU_OPT_K256_WAVES: ok = (v == 3 || v == 4); break;
    case ECGPU_OPT_FB_MEMORY_BUDGET: ok = (v >= 0); break;
    case ECGPU_OPT_LINCOMB_TERM_BY_TERM: ok = (v == 0 || v == 1); break;
    case ECGPU_OPT_SHARED_WINDOW: ok = (v == 0 || v == 8 || v == 16 || v == 20); break;
    case ECGPU_OPT_SHARED_MIN: ok = (v >= 0); break;
    case ECGPU_OPT_SHARED_TABLE_BUDGET: ok = (v >= 0); break;
    case ECGPU_OPT_SHARED_TABLE_BUILDS: ok = (v == 0); break;       // a counter: it can only be reset
    default: return ecgpu_set_err(c, ECGPU_ERR_ARG, "ecgpu_set_option: unknown option %d", option);
  }
  if (!ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "ecgpu_set_option: value %lld is not allowed for option %d", (long long)v, option);
  std::lock_guard<std::mutex> lk(c->mu);
  c->opt[option] = v;
  return ECGPU_OK;
}
int ecgpu_get_option(ecgpu_ctx* c, int option, int64_t* v) {
  if (!c || !v) return ECGPU_ERR_ARG;
  if (option < 0 || option >= ECGPU_OPT_COUNT_) return ecgpu_set_err(c, ECGPU_ERR_ARG, "ecgpu_get_option: unknown option %d", option);
  std::lock_guard<std::mutex> lk(c->mu);
  *v = c->opt[option];
  return ECGPU_OK;
}
int ecgpu_fb_table_bytes(ecgpu_ctx* c, int curve, size_t* bytes, int* widest) {
  if (!c) return ECGPU_ERR_ARG;
  if (curve < 0 || curve > 2) return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "curve %d not supported", curve);
  std::lock_guard<std::mutex> lk(c->mu);
  if (bytes) *bytes = c->fb_bytes[curve];
  if (widest) *widest = c->fb_widest[curve];
  return ECGPU_OK;
}

int ecgpu_host_chunk_schedule(size_t n, size_t pass_units, size_t* sizes, size_t cap) {
  size_t pass = pass_units;
  if (pass > ((size_t)1 << 23)) pass = (size_t)1 << 23;
  if (pass < ((size_t)1 << 20)) pass = (size_t)1 << 20;
  const std::vector<size_t> v = hostpipe::schedule(n, pass / 8, pass, pass / 8, pass / 16);
  for (size_t i = 0; i < v.size() && i < cap && sizes; i++) sizes[i] = v[i];
  return (int)v.size();
}

int ecgpu_debug_workspace(ecgpu_ctx* c, int which, void* host_copy, size_t cap, size_t* bytes) {
  if (!c || !bytes) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  const DevBuf* ws;
  if (which == 0) ws = &c->tab_ws;
  else if (which == 1) ws = &c->ecdsa_ws;
  else if (which == 2) ws = &c->msm_ws;
  else if (which == 3) ws = &c->hash_ws;
  else if (which >= 16 && which < 16 + ecgpu_ctx::NSTAGE) ws = &c->stage[which - 16];
  else return ecgpu_set_err(c, ECGPU_ERR_ARG, "ecgpu_debug_workspace: unknown workspace %d", which);
  void* p = ws->p;
  const size_t sz = ws->cap;
  *bytes = sz;
  if (host_copy && p && sz && cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(host_copy, p, cap < sz ? cap : sz, hipMemcpyDeviceToHost));
  }
  return ECGPU_OK;
}

int ecgpu_host_alloc(ecgpu_ctx* c, size_t bytes, void** out) {
  if (!c || !out) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  *out = nullptr;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
  return ECGPU_OK;
}
int ecgpu_host_free(ecgpu_ctx* c, void* p) {
  if (!c) return ECGPU_ERR_ARG;
  if (!p) return ECGPU_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipHostFree(p));
  return ECGPU_OK;
}

int ecgpu_timer_start(ecgpu_ctx* c) {
  if (!c) return ECGPU_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventRecord(c->ev0, c->stream));
  return ECGPU_OK;
}
int ecgpu_timer_stop(ecgpu_ctx* c, float* ms) {
  if (!c || !ms) return ECGPU_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventRecord(c->ev1, c->stream));
  HIPCHK(c, hipEventSynchronize(c->ev1));
  HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
  return ECGPU_OK;
}

// ---------------------------------------------------------------------------------------------
int ecgpu_field_op_batch(ecgpu_ctx* c, int curve, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n, int mem) {
  if (!c || !a || !out) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  const bool binary = (op == ECGPU_FE_MUL || op == ECGPU_FE_ADD || op == ECGPU_FE_SUB);
  if (binary && !b) return ecgpu_set_err(c, ECGPU_ERR_ARG, "binary field op needs b");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(a, nb), arg_in(binary ? b : nullptr, nb, ARG_OPTIONAL), arg_out(out, nb)};
  return run_batch(c, mem, n, args, 0, [&](void** d, size_t cnt) {
    return ops->field_op(c, op, (const uint32_t*)d[0], (const uint32_t*)d[1], (uint32_t*)d[2], cnt);
  });
}

// scalar field: operands are usually secrets, so their staged copies and the staged results are cleared on every exit path
int ecgpu_scalar_op_batch(ecgpu_ctx* c, int curve, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, uint8_t* ok, size_t n, int mem) {
  if (!c || !a || !out) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (op < ECGPU_SC_MUL || op > ECGPU_SC_SQRT) return ecgpu_set_err(c, ECGPU_ERR_ARG, "unknown scalar op %d", op);
  const bool binary = (op == ECGPU_SC_MUL || op == ECGPU_SC_ADD || op == ECGPU_SC_SUB);
  if (binary && !b) return ecgpu_set_err(c, ECGPU_ERR_ARG, "binary scalar op needs b");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(a, nb, ARG_SECRET), arg_in(binary ? b : nullptr, nb, binary ? ARG_SECRET : ARG_OPTIONAL),
                          arg_out(out, nb, ARG_SECRET), arg_out(ok, 1, ARG_SECRET | ARG_OPTIONAL)};
  return run_batch(c, mem, n, args, 0, [&](void** d, size_t cnt) {
    return ops->scalar_op(c, op, (const uint32_t*)d[0], (const uint32_t*)d[1], (uint32_t*)d[2], (uint8_t*)d[3], cnt);
  });
}
int ecgpu_scalar_reduce_batch(ecgpu_ctx* c, int curve, const uint8_t* in, size_t in_bytes, uint8_t* out, size_t n, int mem, unsigned flags) {
  if (!c || !in || !out) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  const size_t width = ecgpu_field_bytes(curve);
  if (!width) return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "curve %d not supported", curve);
  if (in_bytes < 1 || in_bytes > 2 * width) return ecgpu_set_err(c, ECGPU_ERR_ARG, "in_bytes %zu outside 1 .. %zu", in_bytes, 2 * width);
  if (flags & ~(unsigned)ECGPU_REDUCE_NONZERO) return ecgpu_set_err(c, ECGPU_ERR_ARG, "unknown reduce flags 0x%x", flags);
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(in, in_bytes, ARG_SECRET), arg_out(out, nb, ARG_SECRET)};
  return run_batch(c, mem, n, args, 0, [&](void** d, size_t cnt) {
    return ops->scalar_reduce(c, (const uint8_t*)d[0], in_bytes, (uint32_t*)d[1], cnt, flags);
  });
}

static int point_op(ecgpu_ctx* c, int curve, int op, const uint8_t* p, const uint8_t* q, int q_coords, uint8_t* out, size_t n, int mem) {
  if (!c || !p || !out || (q_coords && !q)) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(p, 3 * nb), arg_in(q, q_coords * nb, q_coords ? 0 : ARG_OPTIONAL), arg_out(out, 3 * nb)};
  return run_batch(c, mem, n, args, 0, [&](void** d, size_t cnt) {
    return ops->point_op(c, op, (const uint32_t*)d[0], (const uint32_t*)d[1], (uint32_t*)d[2], cnt);
  });
}
int ecgpu_point_add_batch(ecgpu_ctx* c, int curve, const uint8_t* p, const uint8_t* q, uint8_t* out, size_t n, int mem) {
  return point_op(c, curve, 0, p, q, 3, out, n, mem);
}
int ecgpu_point_add_mixed_batch(ecgpu_ctx* c, int curve, const uint8_t* p, const uint8_t* q, uint8_t* out, size_t n, int mem) {
  return point_op(c, curve, 1, p, q, 2, out, n, mem);
}
int ecgpu_point_double_batch(ecgpu_ctx* c, int curve, const uint8_t* p, uint8_t* out, size_t n, int mem) {
  return point_op(c, curve, 2, p, nullptr, 0, out, n, mem);
}

int ecgpu_point_eq_batch(ecgpu_ctx* c, int curve, const uint8_t* p, const uint8_t* q, uint8_t* eq, size_t n, int mem) {
  if (!c || !p || !q || !eq) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(p, 3 * nb), arg_in(q, 3 * nb), arg_out(eq, 1)};
  return run_batch(c, mem, n, args, 0, [&](void** d, size_t cnt) {
    return ops->point_eq(c, (const uint32_t*)d[0], (const uint32_t*)d[1], (uint8_t*)d[2], cnt);
  });
}

int ecgpu_batch_normalize(ecgpu_ctx* c, int curve, const uint8_t* p, uint8_t* out_xy, uint8_t* out_inf, size_t n, int mem) {
  if (!c || !p || !out_xy) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(p, 3 * nb), arg_out(out_xy, 2 * nb), arg_out(out_inf, 1, ARG_OPTIONAL)};
  return run_batch(c, mem, n, args, 0, [&](void** d, size_t cnt) {
    return ops->normalize(c, (const uint32_t*)d[0], (uint32_t*)d[1], (uint8_t*)d[2], cnt);
  });
}

// ---------------------------------------------------------------------------------------------
// Shared points (include/ecgpu.h, ECGPU_SHARED_POINTS): `terms` host points that every element of the batch uses.  shared_prepare decides
// between the table path (every point's table in the context's cache, built on a miss; csrc/sharedbase.hpp) and the broadcast path (the
// points replicated in shared_ws for the ordinary launchers) and leaves the call's Plan; everything runs under the context lock the
// entry point holds, and before run_batch: a build and an eviction synchronise the stream.
// ---------------------------------------------------------------------------------------------
namespace shared {
// The size rule, from measurements (profiles/shared_points.txt; one point, device-resident, against the replicated call).
// default_min: the smallest measured batch at which a first call - build and multiplication - beats the replicated call by more than the
// spread of the runs.  rule_width: the width a miss builds - 16-bit windows from the size at which their build and call beat the 8-bit
// table's; 20-bit windows do not pay for their build within 2^22 results, so a miss never picks them (ECGPU_OPT_SHARED_WINDOW does, and
// a cached 20-bit table is used at every size).
static size_t default_min(int curve) { return (size_t)1 << (curve == ECGPU_K256 ? 20 : 18); }
static int rule_width(int curve, size_t n) { return n >= ((size_t)1 << (curve == ECGPU_P384 ? 22 : 20)) ? 16 : 8; }
constexpr int NOMEM = 100;                          // internal: a table did not fit, the caller steps down a width
constexpr int CT_WB = 5;                            // the constant-time kernel's table (fixedbase_ct.hpp)
struct Plan {
  bool table = false;                               // the table path; otherwise `rep` holds the points for the ordinary launchers
  int wb = 0;
  const void* tabs[ECGPU_SHARED_MAX_TERMS] = {};    // nullptr: that term's point is the identity
  uint32_t* rep = nullptr;                          // the points n times: the broadcast path, and a shared key for its prep kernel
  bool valid = true;                                // a shared key that failed validation: the call's answer is all zeros, not an error
};
static bool is_identity(const uint8_t* p, size_t bytes) {
  uint8_t z = 0;
  for (size_t i = 0; i < bytes; i++) z |= p[i];
  return z == 0;
}
static ecgpu_ctx::SharedTable* find(ecgpu_ctx* c, int curve, const uint8_t* key, size_t kb, int wb) {
  for (ecgpu_ctx::SharedTable& t : c->shared_tabs)
    if (t.curve == curve && t.wb == wb && memcmp(t.key, key, kb) == 0) return &t;
  return nullptr;
}
// the point's canonical words, kept behind its table
static const uint32_t* words_of(const ecgpu_ctx::SharedTable& t) { return (const uint32_t*)((const char*)t.p + t.bytes); }
// Frees the least recently used table that this call (`clock`) does not use - of `curve`, or of any curve for curve < 0.  The stream is
// drained first: a kernel of an earlier call may still read the table.
static int evict_one(ecgpu_ctx* c, int curve, uint64_t clock) {
  size_t victim = c->shared_tabs.size();
  for (size_t i = 0; i < c->shared_tabs.size(); i++) {
    const ecgpu_ctx::SharedTable& t = c->shared_tabs[i];
    if (t.used == clock || (curve >= 0 && t.curve != curve)) continue;
    if (victim == c->shared_tabs.size() || t.used < c->shared_tabs[victim].used) victim = i;
  }
  if (victim == c->shared_tabs.size()) return NOMEM;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipFree(c->shared_tabs[victim].p));
  c->shared_bytes -= c->shared_tabs[victim].bytes;
  c->shared_tabs.erase(c->shared_tabs.begin() + victim);
  return 0;
}
// *table = the table of width wb of the point `key` (its words are at d_xy on the device), from the cache or built now.
static int ensure(ecgpu_ctx* c, const ecgpu_curve_ops* ops, int curve, const uint8_t* key, size_t kb, int wb, const uint32_t* d_xy, void* bases,
                  uint64_t clock, const void** table) {
  if (ecgpu_ctx::SharedTable* t = find(c, curve, key, kb, wb)) {
    t->used = clock;
    *table = t->p;
    return 0;
  }
  const size_t bytes = ops->shared_table_bytes(wb);
  if (!bytes) return ecgpu_set_err(c, ECGPU_ERR_ARG, "shared points: no table of %d-bit windows", wb);
  // (like the generator's, the 5-bit table of the constant-time kernel - 53-116 KB - is never refused on the budget's account, though it counts)
  const size_t budget = (size_t)c->opt[ECGPU_OPT_SHARED_TABLE_BUDGET];
  const bool budgeted = wb != CT_WB;
  if (budgeted && bytes > budget) return NOMEM;
  for (;;) {
    size_t of_curve = 0;
    for (const ecgpu_ctx::SharedTable& t : c->shared_tabs) of_curve += t.curve == curve;
    int rc;
    if (of_curve >= ecgpu_ctx::SHARED_TABLES_PER_CURVE) rc = evict_one(c, curve, clock);
    else if (budgeted && c->shared_bytes + bytes > budget) rc = evict_one(c, -1, clock);
    else break;
    if (rc) return rc;
  }
  void* p = nullptr;
  for (;;) {
    const hipError_t e = hipMalloc(&p, bytes + kb);
    if (e == hipSuccess) break;
    if (e != hipErrorOutOfMemory) return ecgpu_set_err(c, ECGPU_ERR_RUNTIME, "shared-point table (%d-bit windows): %s", wb, hipGetErrorString(e));
    (void)hipGetLastError();           // not sticky: the next launch check must not report it
    const int rc = evict_one(c, -1, clock);
    if (rc) return rc;                 // nothing left to free: the caller steps down a width
  }
  int rc = ops->shared_build(c, d_xy, wb, bases, p);
  hipError_t e = rc ? hipSuccess : hipMemcpyAsync((char*)p + bytes, d_xy, kb, hipMemcpyDeviceToDevice, c->stream);
  if (!rc && e == hipSuccess) e = hipStreamSynchronize(c->stream);       // later calls may run on another stream (ecgpu_set_stream)
  if (rc || e != hipSuccess) {
    (void)hipFree(p);
    return rc ? rc : ecgpu_set_err(c, ECGPU_ERR_RUNTIME, "shared-point table (%d-bit windows): %s", wb, hipGetErrorString(e));
  }
  ecgpu_ctx::SharedTable t{p, bytes, curve, wb, clock, {0}};
  memcpy(t.key, key, kb);
  c->shared_tabs.push_back(t);
  c->shared_bytes += bytes;
  c->opt[ECGPU_OPT_SHARED_TABLE_BUILDS]++;
  *table = p;
  return 0;
}
}  // namespace shared

// key_mode: `points` is the one key of ecgpu_ecdsa_verify_batch - plan.rep is always filled (the prep kernel reads a key per element), and a
// key that does not validate is plan.valid = false, not an error.
static int shared_prepare(ecgpu_ctx* c, const ecgpu_curve_ops* ops, int curve, const uint8_t* points, size_t terms, size_t n, unsigned flags, bool key_mode,
                          shared::Plan& plan) {
  const size_t kb = 2 * ecgpu_field_bytes(curve);
  const bool secret = (flags & ECGPU_SECRET_SCALARS) && !(flags & ECGPU_EXACT_REFERENCE);
  bool can_table = !(flags & ECGPU_EXACT_REFERENCE) && terms <= (size_t)ECGPU_SHARED_MAX_TERMS;
  if (can_table && (secret || key_mode) && (terms > 1 || shared::is_identity(points, kb))) can_table = false;
  const uint64_t clock = ++c->shared_clock;
  // a budget that was lowered since the tables were built holds from the next call on
  while (c->shared_bytes > (size_t)c->opt[ECGPU_OPT_SHARED_TABLE_BUDGET]) {
    const int rc = shared::evict_one(c, -1, clock);
    if (rc == shared::NOMEM) break;
    if (rc) return rc;
  }
  const size_t min_n = c->opt[ECGPU_OPT_SHARED_MIN] ? (size_t)c->opt[ECGPU_OPT_SHARED_MIN] : shared::default_min(curve);
  const int pinned = (int)c->opt[ECGPU_OPT_SHARED_WINDOW];
  const int rule = shared::rule_width(curve, n);
  const int build_wb = secret ? shared::CT_WB : pinned ? pinned : rule;
  // the widths a cached table may have to count as a hit: the one a build would pick, a wider one, or - for a batch too small to build - any
  int cand[4], ncand = 0;
  cand[ncand++] = build_wb;
  if (!secret && !pinned)
    for (int w : {20, 16, 8})
      if (w != rule && (w > rule || n < min_n)) cand[ncand++] = w;
  bool hit = false;
  for (int k = 0; can_table && !hit && k < ncand; k++) {
    hit = true;
    for (size_t t = 0; t < terms && hit; t++)
      hit = shared::is_identity(points + t * kb, kb) || shared::find(c, curve, points + t * kb, kb, cand[k]);
    if (!hit) continue;
    plan.wb = cand[k];
    for (size_t t = 0; t < terms; t++) {
      ecgpu_ctx::SharedTable* e = shared::is_identity(points + t * kb, kb) ? nullptr : shared::find(c, curve, points + t * kb, kb, cand[k]);
      if (e) e->used = clock;
      plan.tabs[t] = e ? e->p : nullptr;
    }
  }
  plan.table = hit;
  if (hit && !key_mode) return 0;                  // no copy, no synchronisation
  const bool build = can_table && !hit && n >= min_n;
  const bool replicate = key_mode || (!hit && !build);
  uint32_t* xy;
  uint8_t* okf;
  void* bases;
  int rc = ecgpu_carve(c, c->shared_ws, [&](WsCarver& ws) {
    xy = ws.take<uint32_t>(terms * kb);
    okf = ws.take<uint8_t>(terms);
    bases = ws.take<void>(128 * 96);               // one entry per window: at most 77 (P-384, 5-bit windows) of 96 bytes
    plan.rep = replicate ? ws.take<uint32_t>(n * terms * kb) : nullptr;
  });
  if (rc) return rc;
  const uint32_t* src = xy;
  if (hit) {
    src = shared::words_of(*shared::find(c, curve, points, kb, plan.wb));      // key mode: the key's words are behind its table
  } else {
    std::vector<uint8_t> ok(terms);
    HIPCHK(c, hipMemcpyAsync(xy, points, terms * kb, hipMemcpyHostToDevice, c->stream));
    if ((rc = ops->validate_points(c, xy, okf, terms))) return rc;
    HIPCHK(c, hipMemcpyAsync(ok.data(), okf, terms, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t t = 0; t < terms; t++) {
      if (ok[t]) continue;
      if (!key_mode) return ecgpu_set_err(c, ECGPU_ERR_ARG, "shared point %zu is not a point of the curve (a coordinate not below p, or off the curve)", t);
      plan.valid = false;
    }
  }
  if (build && plan.valid) {
    // the width is picked once, before anything is built: all the call's tables (cached ones included: they stay) must fit the budget together
    int first_wb = build_wb;
    for (; first_wb != shared::CT_WB && first_wb > 8; first_wb = first_wb == 20 ? 16 : 8) {
      size_t need = 0;
      for (size_t t = 0; t < terms; t++) {
        bool counted = shared::is_identity(points + t * kb, kb);
        for (size_t u = 0; u < t && !counted; u++) counted = memcmp(points + u * kb, points + t * kb, kb) == 0;
        if (!counted) need += ops->shared_table_bytes(first_wb);
      }
      if (need <= (size_t)c->opt[ECGPU_OPT_SHARED_TABLE_BUDGET]) break;
    }
    // (what is left to step down for: hipErrorOutOfMemory, and a curve's 16 tables all in use by this call)
    for (int wb = first_wb;;) {
      bool nomem = false;
      for (size_t t = 0; t < terms && !nomem; t++) {
        plan.tabs[t] = nullptr;
        if (shared::is_identity(points + t * kb, kb)) continue;
        rc = shared::ensure(c, ops, curve, points + t * kb, kb, wb, xy + t * (kb / 4), bases, clock, &plan.tabs[t]);
        if (rc == shared::NOMEM) nomem = true;
        else if (rc) return rc;
      }
      plan.wb = wb;
      if (!nomem) break;
      if (wb == shared::CT_WB || wb == 8)
        return ecgpu_set_err(c, ECGPU_ERR_RUNTIME, "shared points: the %d-bit tables of this call fit neither ECGPU_OPT_SHARED_TABLE_BUDGET nor the device's memory", wb);
      wb = wb == 20 ? 16 : 8;
    }
    plan.table = true;
  }
  if (plan.rep && (rc = ops->broadcast_points(c, src, terms, plan.rep, n))) return rc;
  return 0;
}

static int lincomb_impl(ecgpu_ctx* c, int curve, const uint8_t* scalars, const uint8_t* points, int pt_fmt, size_t terms, uint8_t* out, int out_fmt,
                        uint8_t* out_inf, uint8_t* scalar_ok, size_t n, int mem, unsigned flags) {
  if (!c || !scalars || !out) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if ((pt_fmt != ECGPU_PT_AFFINE && pt_fmt != ECGPU_PT_PROJECTIVE) || (out_fmt != ECGPU_PT_AFFINE && out_fmt != ECGPU_PT_PROJECTIVE))
    return ecgpu_set_err(c, ECGPU_ERR_ARG, "bad point format");
  if (terms == 0) return ecgpu_set_err(c, ECGPU_ERR_ARG, "terms must be >= 1");
  if ((flags & ECGPU_SHARED_POINTS) && (!points || pt_fmt != ECGPU_PT_AFFINE))
    return ecgpu_set_err(c, ECGPU_ERR_ARG, "ECGPU_SHARED_POINTS takes `terms` affine points in host memory");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const size_t pin = (pt_fmt == ECGPU_PT_PROJECTIVE ? 3 : 2) * nb, pout = (out_fmt == ECGPU_PT_PROJECTIVE ? 3 : 2) * nb;
  if (flags & ECGPU_SHARED_POINTS) {
    // the points are no per-element buffer: they stay out of the list (the host pipeline must not chunk them) and their tables stand before run_batch
    const unsigned kflags = flags & ~(unsigned)ECGPU_SHARED_POINTS;
    if (terms > 1024) return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "lincomb_batch: at most 1024 terms per combination");
    shared::Plan plan;
    int rc = shared_prepare(c, ops, curve, points, terms, n, kflags, false, plan);
    if (rc) return rc;
    const unsigned sc_secret = (kflags & (ECGPU_EXACT_REFERENCE | ECGPU_SECRET_SCALARS)) ? ARG_SECRET : 0;
    const unsigned out_secret = (kflags & ECGPU_SECRET_SCALARS) ? ARG_SECRET : 0;
    const CallArg args[] = {arg_in(scalars, terms * nb, sc_secret), arg_out(out, pout, out_secret),
                            arg_out(out_fmt == ECGPU_PT_AFFINE ? out_inf : nullptr, 1, ARG_OPTIONAL), arg_out(scalar_ok, 1, ARG_OPTIONAL)};
    const size_t pass = plan.table ? ops->pass_units(c, 0, 1, kflags) : ops->pass_units(c, 1, terms, kflags);
    return run_batch(c, mem, n, args, pass, [&](void** d, size_t cnt) {
      if (d[3]) {
        int rc2 = ops->validate_scalars(c, (const uint32_t*)d[0], (uint8_t*)d[3], cnt, terms);
        if (rc2) return rc2;
      }
      if (plan.table) return ops->shared_lincomb(c, (const uint32_t*)d[0], plan.tabs, plan.wb, terms, (uint32_t*)d[1], out_fmt, (uint8_t*)d[2], cnt, kflags);
      // every chunk reads the replicated points from their start: the rows repeat with period `terms`
      return ops->lincomb(c, (const uint32_t*)d[0], plan.rep, ECGPU_PT_AFFINE, terms, (uint32_t*)d[1], out_fmt, (uint8_t*)d[2], cnt, kflags);
    });
  }
  // the reference schedule is the one meant for secret scalars: their staged copies do not outlive the call; for a secret scalar
  // the product is a secret too
  const unsigned sc_secret = (flags & (ECGPU_EXACT_REFERENCE | ECGPU_SECRET_SCALARS)) ? ARG_SECRET : 0;
  const unsigned out_secret = (flags & ECGPU_SECRET_SCALARS) ? ARG_SECRET : 0;
  const CallArg args[] = {arg_in(scalars, terms * nb, sc_secret), arg_in(points, terms * pin, ARG_OPTIONAL), arg_out(out, pout, out_secret),
                          arg_out(out_fmt == ECGPU_PT_AFFINE ? out_inf : nullptr, 1, ARG_OPTIONAL), arg_out(scalar_ok, 1, ARG_OPTIONAL)};
  return run_batch(c, mem, n, args, ops->pass_units(c, points != nullptr, terms, flags), [&](void** d, size_t cnt) {
    if (d[4]) {
      int rc = ops->validate_scalars(c, (const uint32_t*)d[0], (uint8_t*)d[4], cnt, terms);
      if (rc) return rc;
    }
    return ops->lincomb(c, (const uint32_t*)d[0], (const uint32_t*)d[1], pt_fmt, terms, (uint32_t*)d[2], out_fmt, (uint8_t*)d[3], cnt, flags);
  });
}

int ecgpu_lincomb_batch(ecgpu_ctx* c, int curve, const uint8_t* scalars, const uint8_t* points, int pt_fmt, size_t terms,
                        uint8_t* out, int out_fmt, uint8_t* out_inf, size_t n, int mem, unsigned flags) {
  return lincomb_impl(c, curve, scalars, points, pt_fmt, terms, out, out_fmt, out_inf, nullptr, n, mem, flags);
}
int ecgpu_lincomb_batch_checked(ecgpu_ctx* c, int curve, const uint8_t* scalars, const uint8_t* points, int pt_fmt, size_t terms,
                                uint8_t* out, int out_fmt, uint8_t* out_inf, uint8_t* scalar_ok, size_t n, int mem, unsigned flags) {
  if (!scalar_ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  return lincomb_impl(c, curve, scalars, points, pt_fmt, terms, out, out_fmt, out_inf, scalar_ok, n, mem, flags);
}

int ecgpu_mul_batch(ecgpu_ctx* c, int curve, const uint8_t* scalars, const uint8_t* points, int pt_fmt, uint8_t* out, int out_fmt,
                    uint8_t* out_inf, size_t n, int mem, unsigned flags) {
  return lincomb_impl(c, curve, scalars, points, pt_fmt, 1, out, out_fmt, out_inf, nullptr, n, mem, flags);
}
int ecgpu_mul_batch_checked(ecgpu_ctx* c, int curve, const uint8_t* scalars, const uint8_t* points, int pt_fmt, uint8_t* out, int out_fmt,
                            uint8_t* out_inf, uint8_t* scalar_ok, size_t n, int mem, unsigned flags) {
  if (!scalar_ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  return lincomb_impl(c, curve, scalars, points, pt_fmt, 1, out, out_fmt, out_inf, scalar_ok, n, mem, flags);
}

// `mem` is where the inputs live, `out_mem` where the one result point goes (the device group sums host-resident slices into
// device-resident partial points: group.hip).  The scalars go to staging slot 0, the points to 1, the result to 2.
static int msm_impl(ecgpu_ctx* c, int curve, const uint8_t* scalars, const uint8_t* points, int pt_fmt, size_t n, uint8_t* out, int out_fmt,
                    int mem, int out_mem) {
  if (!c || !out || (n && (!scalars || !points))) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if ((pt_fmt != ECGPU_PT_AFFINE && pt_fmt != ECGPU_PT_PROJECTIVE) || (out_fmt != ECGPU_PT_AFFINE && out_fmt != ECGPU_PT_PROJECTIVE))
    return ecgpu_set_err(c, ECGPU_ERR_ARG, "bad point format");
  ENTER(c, curve);
  const size_t pin = (pt_fmt == ECGPU_PT_PROJECTIVE ? 3 : 2) * nb, pout = (out_fmt == ECGPU_PT_PROJECTIVE ? 3 : 2) * nb;
  void *ds, *dp, *dout;
  int rc;
  if (n == 0) {                              // the empty sum is the identity: affine zeros, projective (0 : 1 : 0)
    if (out_mem == ECGPU_MEM_HOST) {
      memset(out, 0, pout);
      if (out_fmt == ECGPU_PT_PROJECTIVE) out[2 * nb - 1] = 1;
      return ECGPU_OK;
    }
    HIPCHK(c, hipMemsetAsync(out, 0, pout, c->stream));
    if (out_fmt == ECGPU_PT_PROJECTIVE) HIPCHK(c, hipMemsetAsync(out + 2 * nb - 1, 1, 1, c->stream));
    return ECGPU_OK;
  }
  if (mem == ECGPU_MEM_HOST && n >= MSM_PIPE_MIN) {
    // A large sum from host memory is cut into parts that stream through the pipeline's slots (round 3 staged the WHOLE input - 6.4 GB
    // at 2^26 terms - before the first kernel started): part i is summed while part i + 1 uploads; every part leaves ONE projective
    // point on the device and the parts are added up at the end (a sum with unit scalars: same output formatting as one call).
    const std::vector<size_t> sizes = hostpipe::schedule(n, MSM_PIPE_PART / 2, MSM_PIPE_PART, 0, MSM_PIPE_PART / 8);
    const size_t parts = sizes.size();
    if ((rc = stage_reserve(c, 3, parts * 3 * nb))) return rc;
    if ((rc = stage_reserve(c, 4, parts * nb))) return rc;
    uint8_t* partial = (uint8_t*)c->stage[3].p;
    const hostpipe::Arg args[2] = {{scalars, nullptr, nb}, {points, nullptr, pin}};
    rc = hostpipe::run(c, args, 2, sizes, false, [&](int slot, size_t bytes) { return stage_reserve(c, slot, bytes); },
                       [&](void** d, size_t cnt, size_t ci) {
                         return ops->msm(c, (const uint32_t*)d[0], (const uint32_t*)d[1], pt_fmt, cnt, (uint32_t*)(partial + ci * 3 * nb), ECGPU_PT_PROJECTIVE);
                       });
    if (rc) return rc;
    std::vector<uint8_t> ones(parts * nb, 0);
    for (size_t i = 0; i < parts; i++) ones[i * nb + nb - 1] = 1;
    HIPCHK(c, hipMemcpyAsync(c->stage[4].p, ones.data(), parts * nb, hipMemcpyHostToDevice, c->stream));
    if ((rc = stage_arg(c, 2, out, pout, true, out_mem, &dout))) return rc;
    if ((rc = ops->msm(c, (const uint32_t*)c->stage[4].p, (const uint32_t*)partial, ECGPU_PT_PROJECTIVE, parts, (uint32_t*)dout, out_fmt))) return rc;
    if ((rc = unstage_out(c, out, dout, pout, out_mem))) return rc;
    return finish_host(c, ECGPU_MEM_HOST);   // `ones` lives until the stream has been synchronised here
  }
  if ((rc = stage_arg(c, 0, scalars, n * nb, false, mem, &ds))) return rc;
  if ((rc = stage_arg(c, 1, points, n * pin, false, mem, &dp))) return rc;
  if ((rc = stage_arg(c, 2, out, pout, true, out_mem, &dout))) return rc;
  if ((rc = ops->msm(c, (const uint32_t*)ds, (const uint32_t*)dp, pt_fmt, n, (uint32_t*)dout, out_fmt))) return rc;
  if ((rc = unstage_out(c, out, dout, pout, out_mem))) return rc;
  return finish_host(c, (mem == ECGPU_MEM_HOST || out_mem == ECGPU_MEM_HOST) ? ECGPU_MEM_HOST : ECGPU_MEM_DEVICE);    // staged inputs must have left the host buffers
}
int ecgpu_msm(ecgpu_ctx* c, int curve, const uint8_t* scalars, const uint8_t* points, int pt_fmt, size_t n, uint8_t* out, int out_fmt,
              int mem) {
  return msm_impl(c, curve, scalars, points, pt_fmt, n, out, out_fmt, mem, mem);
}


// ---------------------------------------------------------------------------------------------
int ecgpu_validate_scalars(ecgpu_ctx* c, int curve, const uint8_t* scalars, uint8_t* ok, size_t n, int mem) {
  if (!c || !scalars || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(scalars, nb), arg_out(ok, 1)};
  return run_batch(c, mem, n, args, 0, [&](void** d, size_t cnt) { return ops->validate_scalars(c, (const uint32_t*)d[0], (uint8_t*)d[1], cnt, 1); });
}
int ecgpu_validate_points(ecgpu_ctx* c, int curve, const uint8_t* xy, uint8_t* ok, size_t n, int mem) {
  if (!c || !xy || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(xy, 2 * nb), arg_out(ok, 1)};
  return run_batch(c, mem, n, args, 0, [&](void** d, size_t cnt) { return ops->validate_points(c, (const uint32_t*)d[0], (uint8_t*)d[1], cnt); });
}
int ecgpu_decompress_batch(ecgpu_ctx* c, int curve, const uint8_t* x, const uint8_t* y_is_odd, uint8_t* out_xy, uint8_t* ok, size_t n, int mem) {
  if (!c || !x || !y_is_odd || !out_xy || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(x, nb), arg_in(y_is_odd, 1), arg_out(out_xy, 2 * nb), arg_out(ok, 1)};
  return run_batch(c, mem, n, args, 0, [&](void** d, size_t cnt) {
    return ops->decompress(c, (const uint32_t*)d[0], (const uint8_t*)d[1], (uint32_t*)d[2], (uint8_t*)d[3], cnt);
  });
}

int ecgpu_to_bytes_batch(ecgpu_ctx* c, int curve, const uint8_t* points, int pt_fmt, uint8_t* out, size_t n, int mem) {
  if (!c || !points || !out) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (pt_fmt != ECGPU_PT_AFFINE && pt_fmt != ECGPU_PT_PROJECTIVE) return ecgpu_set_err(c, ECGPU_ERR_ARG, "bad point format");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(points, (pt_fmt == ECGPU_PT_PROJECTIVE ? 3 : 2) * nb), arg_out(out, nb + 1)};
  return run_batch(c, mem, n, args, 0, [&](void** d, size_t cnt) { return ops->to_bytes(c, (const uint32_t*)d[0], pt_fmt, (uint8_t*)d[1], cnt); });
}
int ecgpu_from_bytes_batch(ecgpu_ctx* c, int curve, const uint8_t* in, uint8_t* out_xy, uint8_t* ok, size_t n, int mem) {
  if (!c || !in || !out_xy || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(in, nb + 1), arg_out(out_xy, 2 * nb), arg_out(ok, 1)};
  return run_batch(c, mem, n, args, 0, [&](void** d, size_t cnt) { return ops->from_bytes(c, (const uint8_t*)d[0], (uint32_t*)d[1], (uint8_t*)d[2], cnt); });
}

int ecgpu_sec1_encode_batch(ecgpu_ctx* c, int curve, const uint8_t* points, int pt_fmt, int compress, uint8_t* out, size_t n, int mem) {
  if (!c || !points || !out) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (pt_fmt != ECGPU_PT_AFFINE && pt_fmt != ECGPU_PT_PROJECTIVE) return ecgpu_set_err(c, ECGPU_ERR_ARG, "bad point format");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(points, (pt_fmt == ECGPU_PT_PROJECTIVE ? 3 : 2) * nb), arg_out(out, 1 + (compress ? 1 : 2) * nb)};
  return run_batch(c, mem, n, args, 0, [&](void** d, size_t cnt) {
    return ops->sec1_encode(c, (const uint32_t*)d[0], pt_fmt, compress ? 1 : 0, (uint8_t*)d[1], cnt);
  });
}
int ecgpu_sec1_decode_batch(ecgpu_ctx* c, int curve, const uint8_t* in, size_t record_bytes, uint8_t* out_xy, uint8_t* ok, size_t n, int mem) {
  if (!c || !in || !out_xy || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  if (record_bytes != 1 + nb && record_bytes != 1 + 2 * nb)
    return ecgpu_set_err(c, ECGPU_ERR_ARG, "ecgpu_sec1_decode_batch: record_bytes must be %zu (compressed) or %zu (uncompressed)", 1 + nb, 1 + 2 * nb);
  const CallArg args[] = {arg_in(in, record_bytes), arg_out(out_xy, 2 * nb), arg_out(ok, 1)};
  return run_batch(c, mem, n, args, 0, [&](void** d, size_t cnt) {
    return ops->sec1_decode(c, (const uint8_t*)d[0], record_bytes, (uint32_t*)d[1], (uint8_t*)d[2], cnt);
  });
}

// ---------------------------------------------------------------------------------------------
int ecgpu_ecdsa_verify_batch(ecgpu_ctx* c, int curve, const uint8_t* prehash, const uint8_t* sig_rs, const uint8_t* pubkeys_xy, uint8_t* ok,
                             size_t n, int mem, unsigned flags) {
  if (!c || !prehash || !sig_rs || !pubkeys_xy || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  if (flags & ECGPU_SHARED_POINTS) {
    // one key in host memory for the whole batch: it leaves the list, the prep kernel reads its replicated copy (the same rows for every
    // chunk), u2 Q runs on the key's table.  A key the per-element call would reject - invalid, or the identity - and a batch too small
    // to build a table for go through the per-element launcher on the copy: ok = 0 throughout for the former.
    const unsigned kflags = flags & ~(unsigned)ECGPU_SHARED_POINTS;
    shared::Plan plan;
    int rc = shared_prepare(c, ops, curve, pubkeys_xy, 1, n, 0, true, plan);
    if (rc) return rc;
    const CallArg args[] = {arg_in(prehash, nb), arg_in(sig_rs, 2 * nb), arg_out(ok, 1)};
    return run_batch(c, mem, n, args, ops->pass_units(c, plan.table ? 0 : 1, 1, 0), [&](void** d, size_t cnt) {
      if (plan.table)
        return ops->ecdsa_verify_shared(c, (const uint32_t*)d[0], (const uint32_t*)d[1], plan.rep, plan.tabs[0], plan.wb, (uint8_t*)d[2], cnt, kflags);
      return ops->ecdsa_verify(c, (const uint32_t*)d[0], (const uint32_t*)d[1], plan.rep, (uint8_t*)d[2], cnt, kflags);
    });
  }
  const CallArg args[] = {arg_in(prehash, nb), arg_in(sig_rs, 2 * nb), arg_in(pubkeys_xy, 2 * nb), arg_out(ok, 1)};
  return run_batch(c, mem, n, args, ops->pass_units(c, 1, 1, 0), [&](void** d, size_t cnt) {
    return ops->ecdsa_verify(c, (const uint32_t*)d[0], (const uint32_t*)d[1], (const uint32_t*)d[2], (uint8_t*)d[3], cnt, flags);
  });
}
int ecgpu_map_to_curve_batch(ecgpu_ctx* c, int curve, const uint8_t* u, int count, uint8_t* out_xy, uint8_t* out_inf, size_t n, int mem) {
  if (!c || !u || !out_xy) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (count != 1 && count != 2) return ecgpu_set_err(c, ECGPU_ERR_ARG, "count must be 1 (map_to_curve) or 2 (hash_to_curve: Q0 + Q1)");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(u, count * nb), arg_out(out_xy, 2 * nb), arg_out(out_inf, 1, ARG_OPTIONAL)};
  return run_batch(c, mem, n, args, 0, [&](void** d, size_t cnt) {
    return ops->h2c_map(c, (const uint32_t*)d[0], count, (uint32_t*)d[1], (uint8_t*)d[2], cnt);
  });
}
int ecgpu_ecdsa_recover_batch(ecgpu_ctx* c, int curve, const uint8_t* prehash, const uint8_t* sig_rs, const uint8_t* recovery_id,
                              uint8_t* pubkeys_xy, uint8_t* ok, size_t n, int mem, unsigned flags) {
  if (!c || !prehash || !sig_rs || !recovery_id || !pubkeys_xy || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(prehash, nb), arg_in(sig_rs, 2 * nb), arg_in(recovery_id, 1), arg_out(pubkeys_xy, 2 * nb), arg_out(ok, 1)};
  return run_batch(c, mem, n, args, ops->pass_units(c, 1, 1, 0), [&](void** d, size_t cnt) {
    return ops->ecdsa_recover(c, (const uint32_t*)d[0], (const uint32_t*)d[1], (const uint8_t*)d[2], (uint32_t*)d[3], (uint8_t*)d[4], cnt, flags);
  });
}
int ecgpu_schnorr_verify_batch(ecgpu_ctx* c, int curve, const uint8_t* pubkeys_x, const uint8_t* sig_rs, const uint8_t* challenges, uint8_t* ok,
                               size_t n, int mem) {
  if (!c || !pubkeys_x || !sig_rs || !challenges || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(pubkeys_x, nb), arg_in(sig_rs, 2 * nb), arg_in(challenges, nb), arg_out(ok, 1)};
  return run_batch(c, mem, n, args, ops->pass_units(c, 1, 1, 0), [&](void** d, size_t cnt) {
    return ops->schnorr_verify(c, (const uint32_t*)d[0], (const uint32_t*)d[1], (const uint32_t*)d[2], (uint8_t*)d[3], cnt);
  });
}
// staged secret keys and nonces are cleared on every exit path (the signature is public)
int ecgpu_ecdsa_sign_batch(ecgpu_ctx* c, int curve, const uint8_t* secret_d, const uint8_t* nonce_k, const uint8_t* prehash, uint8_t* sig_rs,
                           uint8_t* recovery_id, uint8_t* ok, size_t n, int mem, unsigned flags) {
  if (!c || !secret_d || !nonce_k || !prehash || !sig_rs || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(secret_d, nb, ARG_SECRET), arg_in(nonce_k, nb, ARG_SECRET), arg_in(prehash, nb),
                          arg_out(sig_rs, 2 * nb), arg_out(recovery_id, 1, ARG_OPTIONAL), arg_out(ok, 1)};
  // the dominant kernel is the nonce's generator multiplication, on the schedule CurveOps::ecdsa_sign picks for these flags
  const unsigned fb_flags = (flags & ECGPU_PUBLIC_SCALARS) ? 0u : (flags & ECGPU_EXACT_REFERENCE) ? (unsigned)ECGPU_EXACT_REFERENCE : (unsigned)ECGPU_SECRET_SCALARS;
  return run_batch(c, mem, n, args, ops->pass_units(c, 0, 1, fb_flags), [&](void** d, size_t cnt) {
    return ops->ecdsa_sign(c, (const uint32_t*)d[0], (const uint32_t*)d[1], (const uint32_t*)d[2], (uint32_t*)d[3], (uint8_t*)d[4], (uint8_t*)d[5], cnt,
                           flags);
  });
}

// ---------------------------------------------------------------------------------------------
// deterministic signing (signing_kernels.hpp): the nonce is derived on the device from the key and the digest.  Keys, additional
// data and aux_rand are staged as secrets; a derived nonce leaves the device only through ecgpu_rfc6979_nonce_batch, as a secret too.
// ---------------------------------------------------------------------------------------------
int ecgpu_rfc6979_nonce_batch(ecgpu_ctx* c, int curve, const uint8_t* secret_d, const uint8_t* prehash, const uint8_t* extra, uint8_t* out_k, size_t n,
                              int mem) {
  if (!c || !secret_d || !prehash || !out_k) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(secret_d, nb, ARG_SECRET), arg_in(prehash, nb), arg_in(extra, nb, ARG_SECRET | ARG_OPTIONAL), arg_out(out_k, nb, ARG_SECRET)};
  return run_batch(c, mem, n, args, (size_t)1 << 22, [&](void** d, size_t cnt) {
    return ops->rfc6979_nonce(c, (const uint32_t*)d[0], (const uint32_t*)d[1], (const uint32_t*)d[2], (uint32_t*)d[3], cnt);
  });
}
int ecgpu_ecdsa_sign_prehash_batch(ecgpu_ctx* c, int curve, const uint8_t* secret_d, const uint8_t* prehash, const uint8_t* extra, uint8_t* sig_rs,
                                   uint8_t* recovery_id, uint8_t* ok, size_t n, int mem, unsigned flags) {
  if (!c || !secret_d || !prehash || !sig_rs || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (flags & ECGPU_PUBLIC_SCALARS)
    return ecgpu_set_err(c, ECGPU_ERR_ARG, "ecgpu_ecdsa_sign_prehash_batch: ECGPU_PUBLIC_SCALARS is refused (a nonce derived from the key is never public)");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(secret_d, nb, ARG_SECRET), arg_in(prehash, nb), arg_in(extra, nb, ARG_SECRET | ARG_OPTIONAL),
                          arg_out(sig_rs, 2 * nb), arg_out(recovery_id, 1, ARG_OPTIONAL), arg_out(ok, 1)};
  const unsigned fb_flags = (flags & ECGPU_EXACT_REFERENCE) ? (unsigned)ECGPU_EXACT_REFERENCE : (unsigned)ECGPU_SECRET_SCALARS;
  return run_batch(c, mem, n, args, ops->pass_units(c, 0, 1, fb_flags), [&](void** d, size_t cnt) {
    return ops->ecdsa_sign_prehash(c, (const uint32_t*)d[0], (const uint32_t*)d[1], (const uint32_t*)d[2], (uint32_t*)d[3], (uint8_t*)d[4], (uint8_t*)d[5],
                                   cnt, flags);
  });
}
int ecgpu_schnorr_sign_prehash_batch(ecgpu_ctx* c, int curve, const uint8_t* secret_keys, const uint8_t* prehash, const uint8_t* aux_rand, uint8_t* sig_rs,
                                     uint8_t* pubkeys_x, uint8_t* ok, size_t n, int mem) {
  if (!c || !secret_keys || !prehash || !aux_rand || !sig_rs || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (ecgpu_field_bytes(curve) && curve != ECGPU_K256)
    return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "ecgpu_schnorr_sign_prehash_batch: BIP340 is defined over secp256k1 only");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(secret_keys, nb, ARG_SECRET), arg_in(prehash, 32), arg_in(aux_rand, 32, ARG_SECRET),
                          arg_out(sig_rs, 2 * nb), arg_out(pubkeys_x, nb, ARG_OPTIONAL), arg_out(ok, 1)};
  return run_batch(c, mem, n, args, ops->pass_units(c, 0, 1, ECGPU_SECRET_SCALARS), [&](void** d, size_t cnt) {
    return ops->schnorr_sign_prehash(c, (const uint32_t*)d[0], (const uint32_t*)d[1], (const uint32_t*)d[2], (uint32_t*)d[3], (uint32_t*)d[4], (uint8_t*)d[5], cnt);
  });
}

// the staged secret scalars AND the staged shared values are cleared, whichever way the call ends
int ecgpu_ecdh_batch(ecgpu_ctx* c, int curve, const uint8_t* secret_d, const uint8_t* pubkeys_xy, uint8_t* shared_x, uint8_t* ok, size_t n, int mem) {
  if (!c || !secret_d || !pubkeys_xy || !shared_x || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(secret_d, nb, ARG_SECRET), arg_in(pubkeys_xy, 2 * nb), arg_out(shared_x, nb, ARG_SECRET), arg_out(ok, 1)};
  return run_batch(c, mem, n, args, ops->pass_units(c, 1, 1, ECGPU_SECRET_SCALARS), [&](void** d, size_t cnt) {
    return ops->ecdh(c, (const uint32_t*)d[0], (const uint32_t*)d[1], (uint32_t*)d[2], (uint8_t*)d[3], cnt);
  });
}

// ---------------------------------------------------------------------------------------------
// hash layer (h2c_hash.hpp): everything that starts from message bytes.  The messages of a call share one DST, which travels in the
// kernels' argument block (XmdTail); msg_len is the optional per-message length.
// ---------------------------------------------------------------------------------------------
// the checks every call over messages makes (include/ecgpu.h, "Messages")
static int msgs_enter(ecgpu_ctx* c, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, size_t n, int mem) {
  if (msg_stride && !msgs) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (msg_stride > 0xFFFFFFFFu) return ecgpu_set_err(c, ECGPU_ERR_ARG, "msg_stride %zu does not fit 32 bits", msg_stride);
  if (msg_len && mem == ECGPU_MEM_HOST)
    for (size_t i = 0; i < n; i++)
      if (msg_len[i] > msg_stride) return ecgpu_set_err(c, ECGPU_ERR_ARG, "msg_len[%zu] = %u is above msg_stride = %zu", i, msg_len[i], msg_stride);
  return 0;
}
// the checks every call over messages and a DST makes; fills `tail` for out_len uniform bytes per message
static int xmd_enter(ecgpu_ctx* c, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, const uint8_t* dst, size_t dst_len, size_t out_len,
                     size_t n, int mem, ecgpu::h2c::XmdTail& tail) {
  if (dst_len == 0) return ecgpu_set_err(c, ECGPU_ERR_ARG, "expand_message_xmd: the DST is empty");
  if (!dst || (msg_stride && !msgs)) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (dst_len > 255) return ecgpu_set_err(c, ECGPU_ERR_ARG, "expand_message_xmd: DST of %zu bytes (above 255 the RFC rehashes it: not implemented)", dst_len);
  int rc = msgs_enter(c, msgs, msg_stride, msg_len, n, mem);
  if (rc) return rc;
  ecgpu::h2c::xmd_tail_set(tail, dst, dst_len, out_len);
  return 0;
}
static size_t okm_bytes(int curve) { return curve == ECGPU_P384 ? 72 : 48; }               // FromOkm::Length
static int curve_hash(int curve) { return curve == ECGPU_P384 ? ECGPU_SHA384 : ECGPU_SHA256; }

int ecgpu_expand_message_xmd_batch(ecgpu_ctx* c, int hash, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, const uint8_t* dst,
                                   size_t dst_len, uint8_t* out, size_t out_bytes, size_t n, int mem) {
  if (!c || !out) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (hash != ECGPU_SHA256 && hash != ECGPU_SHA384) return ecgpu_set_err(c, ECGPU_ERR_ARG, "unknown hash %d", hash);
  const size_t digest = hash == ECGPU_SHA384 ? 48 : 32;
  if (out_bytes < 1 || out_bytes > 255 * digest) return ecgpu_set_err(c, ECGPU_ERR_ARG, "out_bytes %zu outside 1 .. %zu (255 digests)", out_bytes, 255 * digest);
  ecgpu::h2c::XmdTail tail;
  int rc = xmd_enter(c, msgs, msg_stride, msg_len, dst, dst_len, out_bytes, n, mem, tail);
  if (rc) return rc;
  if (n == 0) return ECGPU_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  const CallArg args[] = {arg_in(msg_stride ? msgs : nullptr, msg_stride, ARG_OPTIONAL), arg_in(msg_len, 4, ARG_OPTIONAL), arg_out(out, out_bytes)};
  return run_batch(c, mem, n, args, (size_t)1 << 22, [&](void** d, size_t cnt) {
    return ecgpuint_xmd(c, hash, (const uint8_t*)d[0], msg_stride, (const uint32_t*)d[1], tail, (uint8_t*)d[2], cnt);
  });
}
int ecgpu_field_from_okm_batch(ecgpu_ctx* c, int curve, const uint8_t* okm, uint8_t* out, size_t n, int mem) {
  if (!c || !okm || !out) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(okm, okm_bytes(curve)), arg_out(out, nb)};
  return run_batch(c, mem, n, args, (size_t)1 << 22, [&](void** d, size_t cnt) { return ops->field_from_okm(c, (const uint8_t*)d[0], (uint32_t*)d[1], cnt); });
}
int ecgpu_hash_to_curve_batch(ecgpu_ctx* c, int curve, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, const uint8_t* dst, size_t dst_len,
                              int mode, uint8_t* out_xy, uint8_t* out_inf, size_t n, int mem) {
  if (!c || !out_xy) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (mode != ECGPU_H2C_RO && mode != ECGPU_H2C_NU) return ecgpu_set_err(c, ECGPU_ERR_ARG, "unknown hash-to-curve mode %d", mode);
  if (!ecgpu_field_bytes(curve)) return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "curve %d not supported", curve);
  const int count = mode == ECGPU_H2C_RO ? 2 : 1;
  ecgpu::h2c::XmdTail tail;
  int rc = xmd_enter(c, msgs, msg_stride, msg_len, dst, dst_len, count * okm_bytes(curve), n, mem, tail);
  if (rc) return rc;
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(msg_stride ? msgs : nullptr, msg_stride, ARG_OPTIONAL), arg_in(msg_len, 4, ARG_OPTIONAL), arg_out(out_xy, 2 * nb),
                          arg_out(out_inf, 1, ARG_OPTIONAL)};
  return run_batch(c, mem, n, args, (size_t)1 << 22, [&](void** d, size_t cnt) {
    // the field elements go through the pipeline workspace (ecgpu_debug_workspace 1) in the layout the map kernel reads
    uint32_t* u;
    int r = ecgpu_carve(c, c->ecdsa_ws, [&](WsCarver& ws) { u = ws.take<uint32_t>(cnt * count * nb); });
    if (r) return r;
    if ((r = ops->h2c_hash_to_field(c, (const uint8_t*)d[0], msg_stride, (const uint32_t*)d[1], tail, count, u, cnt))) return r;
    return ops->h2c_map(c, u, count, (uint32_t*)d[2], (uint8_t*)d[3], cnt);
  });
}
// derives secret keys: the staged messages and scalars are cleared on every exit path, and so are the uniform bytes in the workspace
int ecgpu_hash_to_scalar_batch(ecgpu_ctx* c, int curve, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, const uint8_t* dst, size_t dst_len,
                               uint8_t* out, size_t n, int mem) {
  if (!c || !out) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (!ecgpu_field_bytes(curve)) return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "curve %d not supported", curve);
  const size_t L = okm_bytes(curve);
  ecgpu::h2c::XmdTail tail;
  int rc = xmd_enter(c, msgs, msg_stride, msg_len, dst, dst_len, L, n, mem, tail);
  if (rc) return rc;
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(msg_stride ? msgs : nullptr, msg_stride, ARG_SECRET | ARG_OPTIONAL), arg_in(msg_len, 4, ARG_OPTIONAL), arg_out(out, nb, ARG_SECRET)};
  return run_batch(c, mem, n, args, (size_t)1 << 22, [&](void** d, size_t cnt) {
    uint8_t* okm;
    int r = ecgpu_carve(c, c->ecdsa_ws, [&](WsCarver& ws) { okm = ws.take<uint8_t>(cnt * L); });
    if (r) return r;
    StreamWipe okm_wipe{c, okm, cnt * L};
    if ((r = ecgpuint_xmd(c, curve_hash(curve), (const uint8_t*)d[0], msg_stride, (const uint32_t*)d[1], tail, okm, cnt))) return r;
    return ops->scalar_reduce(c, okm, L, (uint32_t*)d[2], cnt, 0);
  });
}
int ecgpu_schnorr_verify_prehash_batch(ecgpu_ctx* c, int curve, const uint8_t* pubkeys_x, const uint8_t* sig_rs, const uint8_t* prehash, uint8_t* ok,
                                       size_t n, int mem) {
  if (!c || !pubkeys_x || !sig_rs || !prehash || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (ecgpu_field_bytes(curve) && curve != ECGPU_K256)
    return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "ecgpu_schnorr_verify_prehash_batch: BIP340 is defined over secp256k1 only");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(pubkeys_x, nb), arg_in(sig_rs, 2 * nb), arg_in(prehash, 32), arg_out(ok, 1)};
  return run_batch(c, mem, n, args, ops->pass_units(c, 1, 1, 0), [&](void** d, size_t cnt) {
    uint32_t* e;
    int r = ecgpu_carve(c, c->hash_ws, [&](WsCarver& ws) { e = ws.take<uint32_t>(cnt * 32); });
    if (r) return r;
    if ((r = ops->schnorr_challenge(c, (const uint32_t*)d[0], (const uint32_t*)d[1], (const uint32_t*)d[2], e, cnt))) return r;
    return ops->schnorr_verify(c, (const uint32_t*)d[0], (const uint32_t*)d[1], e, (uint8_t*)d[3], cnt);
  });
}

// ---------------------------------------------------------------------------------------------
// message level (include/ecgpu.h, "from message bytes"): the digest kernel writes the digest of every message - the curve's own, or
// for the *_digest_batch calls a chosen one of the same size - into the hash workspace, then the prehash form's launcher runs on it.
// Messages and digests are public: nothing of them is wiped.
// ---------------------------------------------------------------------------------------------
int ecgpu_digest_batch(ecgpu_ctx* c, int hash, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, uint8_t* out, size_t n, int mem) {
  if (!c || !out) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (!ecgpu_hash_bytes(hash)) return ecgpu_set_err(c, ECGPU_ERR_ARG, "unknown hash %d", hash);
  if (mem == ECGPU_MEM_DEVICE && ((uintptr_t)out & 3u)) return ecgpu_set_err(c, ECGPU_ERR_ARG, "ecgpu_digest_batch: device-resident digests are 4-byte aligned");
  int rc = msgs_enter(c, msgs, msg_stride, msg_len, n, mem);
  if (rc) return rc;
  if (n == 0) return ECGPU_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  const CallArg args[] = {arg_in(msg_stride ? msgs : nullptr, msg_stride, ARG_OPTIONAL), arg_in(msg_len, 4, ARG_OPTIONAL), arg_out(out, ecgpu_hash_bytes(hash))};
  return run_batch(c, mem, n, args, (size_t)1 << 22, [&](void** d, size_t cnt) {
    return ecgpuint_digest(c, hash, (const uint8_t*)d[0], msg_stride, (const uint32_t*)d[1], (uint32_t*)d[2], cnt);
  });
}
// z = cnt digests of `hash` in the hash workspace (the prehash launchers carve ecdsa_ws, never hash_ws); the rows are field-sized
static int digest_to_ws(ecgpu_ctx* c, int curve, int hash, const void* msgs, size_t msg_stride, const void* msg_len, size_t cnt, uint32_t** z, uint32_t** more = nullptr) {
  const size_t nb = ecgpu_field_bytes(curve);
  int rc = ecgpu_carve(c, c->hash_ws, [&](WsCarver& ws) {
    *z = ws.take<uint32_t>(cnt * nb);
    if (more) *more = ws.take<uint32_t>(cnt * nb);
  });
  if (rc) return rc;
  return ecgpuint_digest(c, hash, (const uint8_t*)msgs, msg_stride, (const uint32_t*)msg_len, *z, cnt);
}
static const char* hash_name(int hash) {
  switch (hash) {
    case ECGPU_SHA256: return "SHA-256";
    case ECGPU_SHA384: return "SHA-384";
    case ECGPU_KECCAK256: return "Keccak-256";
    case ECGPU_SHA3_256: return "SHA3-256";
    case ECGPU_SHA3_384: return "SHA3-384";
    default: return "unknown";
  }
}
static const char* curve_name(int curve) { return curve == ECGPU_K256 ? "secp256k1" : curve == ECGPU_P256 ? "P-256" : curve == ECGPU_P384 ? "P-384" : "unknown"; }
// the reference's bound D: Digest<OutputSize = FieldBytesSize<C>>: the digest fills the field (an unknown curve is ENTER's to refuse)
static int hash_fits(ecgpu_ctx* c, const char* what, int curve, int hash) {
  const size_t hb = ecgpu_hash_bytes(hash), nb = ecgpu_field_bytes(curve);
  if (!hb) return ecgpu_set_err(c, ECGPU_ERR_ARG, "%s: unknown hash %d", what, hash);
  if (nb && hb != nb)
    return ecgpu_set_err(c, ECGPU_ERR_ARG, "%s: %s gives %zu bytes, %s takes a digest of %zu (hash %d, curve %d)", what, hash_name(hash), hb, curve_name(curve), nb, hash, curve);
  return 0;
}
// sign / verify / recover from message bytes on `hash`: the *_msg_batch calls are the case hash = curve_hash(curve)
static int sign_from_msgs(ecgpu_ctx* c, const char* what, int curve, int hash, const uint8_t* secret_d, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len,
                          const uint8_t* extra, uint8_t* sig_rs, uint8_t* recovery_id, uint8_t* ok, size_t n, int mem, unsigned flags) {
  if (!c || !secret_d || !sig_rs || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  int rc = hash_fits(c, what, curve, hash);
  if (rc) return rc;
  if (flags & ECGPU_PUBLIC_SCALARS)
    return ecgpu_set_err(c, ECGPU_ERR_ARG, "%s: ECGPU_PUBLIC_SCALARS is refused (a nonce derived from the key is never public)", what);
  if ((rc = msgs_enter(c, msgs, msg_stride, msg_len, n, mem))) return rc;
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(secret_d, nb, ARG_SECRET), arg_in(msg_stride ? msgs : nullptr, msg_stride, ARG_OPTIONAL), arg_in(msg_len, 4, ARG_OPTIONAL),
                          arg_in(extra, nb, ARG_SECRET | ARG_OPTIONAL), arg_out(sig_rs, 2 * nb), arg_out(recovery_id, 1, ARG_OPTIONAL), arg_out(ok, 1)};
  const unsigned fb_flags = (flags & ECGPU_EXACT_REFERENCE) ? (unsigned)ECGPU_EXACT_REFERENCE : (unsigned)ECGPU_SECRET_SCALARS;
  return run_batch(c, mem, n, args, ops->pass_units(c, 0, 1, fb_flags), [&](void** d, size_t cnt) {
    uint32_t* z;
    int r = digest_to_ws(c, curve, hash, d[1], msg_stride, d[2], cnt, &z);
    if (r) return r;
    return ops->ecdsa_sign_prehash(c, (const uint32_t*)d[0], z, (const uint32_t*)d[3], (uint32_t*)d[4], (uint8_t*)d[5], (uint8_t*)d[6], cnt, flags);
  });
}
static int verify_from_msgs(ecgpu_ctx* c, const char* what, int curve, int hash, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, const uint8_t* sig_rs,
                            const uint8_t* pubkeys_xy, uint8_t* ok, size_t n, int mem, unsigned flags) {
  if (!c || !sig_rs || !pubkeys_xy || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (flags & ECGPU_SHARED_POINTS) return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "%s takes one key per element: ECGPU_SHARED_POINTS is for ecgpu_ecdsa_verify_batch", what);
  int rc = hash_fits(c, what, curve, hash);
  if (rc) return rc;
  if ((rc = msgs_enter(c, msgs, msg_stride, msg_len, n, mem))) return rc;
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(msg_stride ? msgs : nullptr, msg_stride, ARG_OPTIONAL), arg_in(msg_len, 4, ARG_OPTIONAL), arg_in(sig_rs, 2 * nb),
                          arg_in(pubkeys_xy, 2 * nb), arg_out(ok, 1)};
  return run_batch(c, mem, n, args, ops->pass_units(c, 1, 1, 0), [&](void** d, size_t cnt) {
    uint32_t* z;
    int r = digest_to_ws(c, curve, hash, d[0], msg_stride, d[1], cnt, &z);
    if (r) return r;
    return ops->ecdsa_verify(c, z, (const uint32_t*)d[2], (const uint32_t*)d[3], (uint8_t*)d[4], cnt, flags);
  });
}
static int recover_from_msgs(ecgpu_ctx* c, const char* what, int curve, int hash, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, const uint8_t* sig_rs,
                             const uint8_t* recovery_id, uint8_t* pubkeys_xy, uint8_t* ok, size_t n, int mem, unsigned flags) {
  if (!c || !sig_rs || !recovery_id || !pubkeys_xy || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  int rc = hash_fits(c, what, curve, hash);
  if (rc) return rc;
  if ((rc = msgs_enter(c, msgs, msg_stride, msg_len, n, mem))) return rc;
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(msg_stride ? msgs : nullptr, msg_stride, ARG_OPTIONAL), arg_in(msg_len, 4, ARG_OPTIONAL), arg_in(sig_rs, 2 * nb),
                          arg_in(recovery_id, 1), arg_out(pubkeys_xy, 2 * nb), arg_out(ok, 1)};
  return run_batch(c, mem, n, args, ops->pass_units(c, 1, 1, 0), [&](void** d, size_t cnt) {
    uint32_t* z;
    int r = digest_to_ws(c, curve, hash, d[0], msg_stride, d[1], cnt, &z);
    if (r) return r;
    return ops->ecdsa_recover(c, z, (const uint32_t*)d[2], (const uint8_t*)d[3], (uint32_t*)d[4], (uint8_t*)d[5], cnt, flags);
  });
}
int ecgpu_ecdsa_sign_msg_batch(ecgpu_ctx* c, int curve, const uint8_t* secret_d, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len,
                               const uint8_t* extra, uint8_t* sig_rs, uint8_t* recovery_id, uint8_t* ok, size_t n, int mem, unsigned flags) {
  return sign_from_msgs(c, "ecgpu_ecdsa_sign_msg_batch", curve, curve_hash(curve), secret_d, msgs, msg_stride, msg_len, extra, sig_rs, recovery_id, ok, n, mem, flags);
}
int ecgpu_ecdsa_verify_msg_batch(ecgpu_ctx* c, int curve, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, const uint8_t* sig_rs,
                                 const uint8_t* pubkeys_xy, uint8_t* ok, size_t n, int mem, unsigned flags) {
  return verify_from_msgs(c, "ecgpu_ecdsa_verify_msg_batch", curve, curve_hash(curve), msgs, msg_stride, msg_len, sig_rs, pubkeys_xy, ok, n, mem, flags);
}
int ecgpu_ecdsa_recover_msg_batch(ecgpu_ctx* c, int curve, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, const uint8_t* sig_rs,
                                  const uint8_t* recovery_id, uint8_t* pubkeys_xy, uint8_t* ok, size_t n, int mem, unsigned flags) {
  return recover_from_msgs(c, "ecgpu_ecdsa_recover_msg_batch", curve, curve_hash(curve), msgs, msg_stride, msg_len, sig_rs, recovery_id, pubkeys_xy, ok, n, mem, flags);
}
// DigestSigner / RandomizedDigestSigner, DigestVerifier and recover_from_digest on a digest of the field's size (include/ecgpu.h)
int ecgpu_ecdsa_sign_digest_batch(ecgpu_ctx* c, int curve, int hash, const uint8_t* secret_d, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len,
                                  const uint8_t* extra, uint8_t* sig_rs, uint8_t* recovery_id, uint8_t* ok, size_t n, int mem, unsigned flags) {
  return sign_from_msgs(c, "ecgpu_ecdsa_sign_digest_batch", curve, hash, secret_d, msgs, msg_stride, msg_len, extra, sig_rs, recovery_id, ok, n, mem, flags);
}
int ecgpu_ecdsa_verify_digest_batch(ecgpu_ctx* c, int curve, int hash, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, const uint8_t* sig_rs,
                                    const uint8_t* pubkeys_xy, uint8_t* ok, size_t n, int mem, unsigned flags) {
  return verify_from_msgs(c, "ecgpu_ecdsa_verify_digest_batch", curve, hash, msgs, msg_stride, msg_len, sig_rs, pubkeys_xy, ok, n, mem, flags);
}
int ecgpu_ecdsa_recover_digest_batch(ecgpu_ctx* c, int curve, int hash, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, const uint8_t* sig_rs,
                                     const uint8_t* recovery_id, uint8_t* pubkeys_xy, uint8_t* ok, size_t n, int mem, unsigned flags) {
  return recover_from_msgs(c, "ecgpu_ecdsa_recover_digest_batch", curve, hash, msgs, msg_stride, msg_len, sig_rs, recovery_id, pubkeys_xy, ok, n, mem, flags);
}
// aux_rand == NULL is the reference's Default::default(), 32 zero bytes per key: the hash workspace holds them behind the digests
int ecgpu_schnorr_sign_msg_batch(ecgpu_ctx* c, int curve, const uint8_t* secret_keys, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len,
                                 const uint8_t* aux_rand, uint8_t* sig_rs, uint8_t* pubkeys_x, uint8_t* ok, size_t n, int mem) {
  if (!c || !secret_keys || !sig_rs || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (ecgpu_field_bytes(curve) && curve != ECGPU_K256)
    return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "ecgpu_schnorr_sign_msg_batch: BIP340 is defined over secp256k1 only");
  int rc = msgs_enter(c, msgs, msg_stride, msg_len, n, mem);
  if (rc) return rc;
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(secret_keys, nb, ARG_SECRET), arg_in(msg_stride ? msgs : nullptr, msg_stride, ARG_OPTIONAL), arg_in(msg_len, 4, ARG_OPTIONAL),
                          arg_in(aux_rand, 32, ARG_SECRET | ARG_OPTIONAL), arg_out(sig_rs, 2 * nb), arg_out(pubkeys_x, nb, ARG_OPTIONAL), arg_out(ok, 1)};
  return run_batch(c, mem, n, args, ops->pass_units(c, 0, 1, ECGPU_SECRET_SCALARS), [&](void** d, size_t cnt) {
    uint32_t *m, *zero_aux = nullptr;
    int r = digest_to_ws(c, curve, ECGPU_SHA256, d[1], msg_stride, d[2], cnt, &m, d[3] ? nullptr : &zero_aux);
    if (r) return r;
    if (zero_aux) HIPCHK(c, hipMemsetAsync(zero_aux, 0, cnt * 32, c->stream));
    return ops->schnorr_sign_prehash(c, (const uint32_t*)d[0], m, d[3] ? (const uint32_t*)d[3] : zero_aux, (uint32_t*)d[4], (uint32_t*)d[5], (uint8_t*)d[6], cnt);
  });
}
int ecgpu_schnorr_verify_msg_batch(ecgpu_ctx* c, int curve, const uint8_t* pubkeys_x, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len,
                                   const uint8_t* sig_rs, uint8_t* ok, size_t n, int mem) {
  if (!c || !pubkeys_x || !sig_rs || !ok) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (ecgpu_field_bytes(curve) && curve != ECGPU_K256)
    return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "ecgpu_schnorr_verify_msg_batch: BIP340 is defined over secp256k1 only");
  int rc = msgs_enter(c, msgs, msg_stride, msg_len, n, mem);
  if (rc) return rc;
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  const CallArg args[] = {arg_in(pubkeys_x, nb), arg_in(msg_stride ? msgs : nullptr, msg_stride, ARG_OPTIONAL), arg_in(msg_len, 4, ARG_OPTIONAL),
                          arg_in(sig_rs, 2 * nb), arg_out(ok, 1)};
  return run_batch(c, mem, n, args, ops->pass_units(c, 1, 1, 0), [&](void** d, size_t cnt) {
    // the digests and the challenges live through schnorr_verify, which carves ecdsa_ws: both come from ONE carve of hash_ws
    uint32_t *m, *e;
    int r = digest_to_ws(c, curve, ECGPU_SHA256, d[1], msg_stride, d[2], cnt, &m, &e);
    if (r) return r;
    if ((r = ops->schnorr_challenge(c, (const uint32_t*)d[0], (const uint32_t*)d[3], m, e, cnt))) return r;
    return ops->schnorr_verify(c, (const uint32_t*)d[0], (const uint32_t*)d[3], e, (uint8_t*)d[4], cnt);
  });
}

// ---------------------------------------------------------------------------------------------
// BIP340 batch verification (include/ecgpu.h, "batch verification"; csrc/schnorr_batch_kernels.hpp).  Every chunk run_batch hands over
// is one equation of its own (ops->schnorr_batch_verify), with the coefficients of its elements' indices in the caller's batch; the
// verdict is the AND over the chunks.  Each equation synchronises the stream, so the chunks of a host batch of PIPE_MIN elements and
// more do not overlap their copies with the kernels of the next one.  Nothing here is secret: nothing is wiped.
// ---------------------------------------------------------------------------------------------
struct SchnorrBatch {
  ecgpu_ctx* c;
  const ecgpu_curve_ops* ops;
  unsigned flags;
  bool equation;         // false: the per-signature pipeline (batches below ECGPU_SCHNORR_BATCH_MIN, where the equation does not win)
  uint8_t seed[32];
  size_t done = 0;       // elements of the chunks so far: run_batch launches them in order
  int all = 1;
  // one chunk whose challenges e are ready
  int chunk(const void* px, const void* sig, const uint32_t* e, void* ok, size_t cnt) {
    if (!equation) return ops->schnorr_verify(c, (const uint32_t*)px, (const uint32_t*)sig, e, (uint8_t*)ok, cnt);
    int verdict = 0;
    const int r = ops->schnorr_batch_verify(c, (const uint32_t*)px, (const uint32_t*)sig, e, (uint8_t*)ok, cnt, (uint64_t)done, seed, flags, &verdict);
    if (r) return r;
    done += cnt;
    all &= verdict;
    return 0;
  }
};
// the checks the three forms share (before the context's lock is taken); *all_valid = 1 for the empty batch
static int schnorr_batch_enter(ecgpu_ctx* c, int curve, const void* pubkeys_x, const void* sig_rs, const void* ok, int* all_valid, size_t n, unsigned flags) {
  if (!c || !pubkeys_x || !sig_rs) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (flags & ~(unsigned)(ECGPU_BATCH_VERDICT_ONLY | ECGPU_BATCH_EQUATION_ALWAYS)) return ecgpu_set_err(c, ECGPU_ERR_ARG, "ecgpu_schnorr_batch_verify: unknown flags 0x%x", flags);
  if (!ok && !(flags & ECGPU_BATCH_VERDICT_ONLY)) return ecgpu_set_err(c, ECGPU_ERR_ARG, "ecgpu_schnorr_batch_verify: ok may be NULL with ECGPU_BATCH_VERDICT_ONLY only");
  if (ecgpu_field_bytes(curve) && curve != ECGPU_K256)
    return ecgpu_set_err(c, ECGPU_ERR_UNSUPPORTED, "ecgpu_schnorr_batch_verify: BIP340 is defined over secp256k1 only");
  if (n == 0 && all_valid) *all_valid = 1;
  return ECGPU_OK;
}
// routing and the seed (the caller's, or 32 bytes of getrandom(2))
static int schnorr_batch_begin(SchnorrBatch& b, const uint8_t* seed32, const void* ok, size_t n) {
  b.equation = (b.flags & ECGPU_BATCH_EQUATION_ALWAYS) || !ok || n >= ECGPU_SCHNORR_BATCH_MIN;
  if (seed32) { memcpy(b.seed, seed32, 32); return 0; }
  for (size_t got = 0; b.equation && got < 32;) {
    const ssize_t r = getrandom(b.seed + got, 32 - got, 0);
    if (r < 0 && errno == EINTR) continue;
    if (r <= 0) return ecgpu_set_err(b.c, ECGPU_ERR_RUNTIME, "ecgpu_schnorr_batch_verify: getrandom failed (errno %d) and no seed was given", errno);
    got += (size_t)r;
  }
  return 0;
}
// after run_batch: the stream is synchronised and the verdict handed out (per-signature routing: the AND over ok)
static int schnorr_batch_end(SchnorrBatch& b, const uint8_t* ok, int* all_valid, size_t n, int mem) {
  ecgpu_ctx* c = b.c;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!b.equation) {
    std::vector<uint8_t> copy;
    if (mem == ECGPU_MEM_DEVICE) {
      copy.resize(n);
      HIPCHK(c, hipMemcpy(copy.data(), ok, n, hipMemcpyDeviceToHost));
      ok = copy.data();
    }
    for (size_t i = 0; i < n; i++) b.all &= ok[i] == 1;
  }
  if (all_valid) *all_valid = b.all;
  return ECGPU_OK;
}
static constexpr size_t SCHNORR_BATCH_PASS = (size_t)1 << 22;

int ecgpu_schnorr_batch_verify(ecgpu_ctx* c, int curve, const uint8_t* pubkeys_x, const uint8_t* sig_rs, const uint8_t* challenges, const uint8_t* seed32,
                               uint8_t* ok, int* all_valid, size_t n, int mem, unsigned flags) {
  int rc = schnorr_batch_enter(c, curve, pubkeys_x, sig_rs, ok, all_valid, n, flags);
  if (rc) return rc;
  if (!challenges) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  SchnorrBatch b{c, ops, flags};
  if ((rc = schnorr_batch_begin(b, seed32, ok, n))) return rc;
  const CallArg args[] = {arg_in(pubkeys_x, nb), arg_in(sig_rs, 2 * nb), arg_in(challenges, nb), arg_out(ok, 1, ARG_OPTIONAL)};
  rc = run_batch(c, mem, n, args, SCHNORR_BATCH_PASS, [&](void** d, size_t cnt) { return b.chunk(d[0], d[1], (const uint32_t*)d[2], d[3], cnt); });
  return rc ? rc : schnorr_batch_end(b, ok, all_valid, n, mem);
}
int ecgpu_schnorr_batch_verify_prehash(ecgpu_ctx* c, int curve, const uint8_t* pubkeys_x, const uint8_t* sig_rs, const uint8_t* prehash, const uint8_t* seed32,
                                       uint8_t* ok, int* all_valid, size_t n, int mem, unsigned flags) {
  int rc = schnorr_batch_enter(c, curve, pubkeys_x, sig_rs, ok, all_valid, n, flags);
  if (rc) return rc;
  if (!prehash) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  SchnorrBatch b{c, ops, flags};
  if ((rc = schnorr_batch_begin(b, seed32, ok, n))) return rc;
  const CallArg args[] = {arg_in(pubkeys_x, nb), arg_in(sig_rs, 2 * nb), arg_in(prehash, 32), arg_out(ok, 1, ARG_OPTIONAL)};
  rc = run_batch(c, mem, n, args, SCHNORR_BATCH_PASS, [&](void** d, size_t cnt) {
    uint32_t* e;
    int r = ecgpu_carve(c, c->hash_ws, [&](WsCarver& ws) { e = ws.take<uint32_t>(cnt * 32); });
    if (r) return r;
    if ((r = ops->schnorr_challenge(c, (const uint32_t*)d[0], (const uint32_t*)d[1], (const uint32_t*)d[2], e, cnt))) return r;
    return b.chunk(d[0], d[1], e, d[3], cnt);
  });
  return rc ? rc : schnorr_batch_end(b, ok, all_valid, n, mem);
}
int ecgpu_schnorr_batch_verify_msg(ecgpu_ctx* c, int curve, const uint8_t* pubkeys_x, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len,
                                   const uint8_t* sig_rs, const uint8_t* seed32, uint8_t* ok, int* all_valid, size_t n, int mem, unsigned flags) {
  int rc = schnorr_batch_enter(c, curve, pubkeys_x, sig_rs, ok, all_valid, n, flags);
  if (rc) return rc;
  if ((rc = msgs_enter(c, msgs, msg_stride, msg_len, n, mem))) return rc;
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  SchnorrBatch b{c, ops, flags};
  if ((rc = schnorr_batch_begin(b, seed32, ok, n))) return rc;
  const CallArg args[] = {arg_in(pubkeys_x, nb), arg_in(msg_stride ? msgs : nullptr, msg_stride, ARG_OPTIONAL), arg_in(msg_len, 4, ARG_OPTIONAL),
                          arg_in(sig_rs, 2 * nb), arg_out(ok, 1, ARG_OPTIONAL)};
  rc = run_batch(c, mem, n, args, SCHNORR_BATCH_PASS, [&](void** d, size_t cnt) {
    uint32_t *m, *e;
    int r = digest_to_ws(c, curve, ECGPU_SHA256, d[1], msg_stride, d[2], cnt, &m, &e);
    if (r) return r;
    if ((r = ops->schnorr_challenge(c, (const uint32_t*)d[0], (const uint32_t*)d[3], m, e, cnt))) return r;
    return b.chunk(d[0], d[3], e, d[4], cnt);
  });
  return rc ? rc : schnorr_batch_end(b, ok, all_valid, n, mem);
}

int ecgpu_synth_scalars(ecgpu_ctx* c, int curve, uint64_t seed, uint64_t first, uint8_t* d_scalars, size_t n) {
  if (!c || !d_scalars) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  return ops->synth_scalars(c, seed, first, (uint32_t*)d_scalars, n);
}
int ecgpu_synth_points(ecgpu_ctx* c, int curve, uint64_t seed, uint64_t first, uint8_t* d_points, size_t n) {
  if (!c || !d_points) return ecgpu_set_err(c, ECGPU_ERR_ARG, "null argument");
  if (n == 0) return ECGPU_OK;
  ENTER(c, curve);
  return ops->synth_points(c, seed, first, (uint32_t*)d_points, n);
}

}  // extern "C"

// internal (C++ linkage: not exported, csrc/ecgpu.map): ecgpu_msm with the inputs and the result in different kinds of memory
int ecgpuint_msm_mixed(ecgpu_ctx* c, int curve, const uint8_t* scalars, const uint8_t* points, int pt_fmt, size_t n, uint8_t* out, int out_fmt,
                       int mem_in, int mem_out) {
  return msm_impl(c, curve, scalars, points, pt_fmt, n, out, out_fmt, mem_in, mem_out);
}
