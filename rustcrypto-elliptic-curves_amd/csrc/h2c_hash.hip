// expand_message_xmd to raw bytes and the plain digest: the kernels of the hash layer that no curve owns (the fused hash_to_field
// kernels are instantiated with their curves in ops_*.hip).
#include "ecgpu_internal.hpp"
#include "h2c_hash.hpp"
using namespace ecgpu;

int ecgpuint_xmd(ecgpu_ctx* c, int hash, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, const h2c::XmdTail& tail, uint8_t* out, size_t n) {
  const unsigned g = ecgpu_grid_for(c, n, 8);
  switch (hash) {
    case ECGPU_SHA256: hipLaunchKernelGGL((h2c::xmd_kernel<sha2::Sha256>), dim3(g), dim3(256), 0, c->stream, msgs, msg_stride, msg_len, tail, out, n); break;
    case ECGPU_SHA384: hipLaunchKernelGGL((h2c::xmd_kernel<sha2::Sha384>), dim3(g), dim3(256), 0, c->stream, msgs, msg_stride, msg_len, tail, out, n); break;
    default: return ecgpu_set_err(c, ECGPU_ERR_ARG, "unknown hash %d", hash);
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}

int ecgpuint_digest(ecgpu_ctx* c, int hash, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, uint32_t* out, size_t n) {
  const unsigned g = ecgpu_grid_for(c, n, 8);
  switch (hash) {
    case ECGPU_SHA256: hipLaunchKernelGGL((h2c::digest_kernel<sha2::Sha256>), dim3(g), dim3(256), 0, c->stream, msgs, msg_stride, msg_len, out, n); break;
    case ECGPU_SHA384: hipLaunchKernelGGL((h2c::digest_kernel<sha2::Sha384>), dim3(g), dim3(256), 0, c->stream, msgs, msg_stride, msg_len, out, n); break;
    default: return ecgpuint_keccak_digest(c, hash, msgs, msg_stride, msg_len, out, n);                    // the sponge family, or "unknown hash"
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}
