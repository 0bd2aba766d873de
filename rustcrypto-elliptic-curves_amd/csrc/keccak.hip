// The sponge digests (keccak.hpp) of ecgpu_digest_batch and of the ecgpu_ecdsa_*_digest_batch calls: a translation unit of its own,
// so that the SHA-2 kernels of h2c_hash.hip are what they were.
#include "ecgpu_internal.hpp"
#include "h2c_hash.hpp"
#include "keccak.hpp"
using namespace ecgpu;

// plain digests: out[i] = the DIGEST_BYTES of message i (rows 4-byte aligned); the shape of h2c::digest_kernel
template <class H>
__global__ void __launch_bounds__(256) keccak_digest_kernel(const uint8_t* msgs, size_t msg_stride, const u32* msg_len, u32* out, size_t n) {
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T)
    keccak::digest_words<H>(out + i * (H::DIGEST_BYTES / 4), msgs + i * msg_stride, h2c::message_length(msg_len, i, msg_stride));
}

int ecgpuint_keccak_digest(ecgpu_ctx* c, int hash, const uint8_t* msgs, size_t msg_stride, const uint32_t* msg_len, uint32_t* out, size_t n) {
  const unsigned g = ecgpu_grid_for(c, n, 8);
  switch (hash) {
    case ECGPU_KECCAK256: hipLaunchKernelGGL((keccak_digest_kernel<keccak::Keccak256>), dim3(g), dim3(256), 0, c->stream, msgs, msg_stride, msg_len, out, n); break;
    case ECGPU_SHA3_256: hipLaunchKernelGGL((keccak_digest_kernel<keccak::Sha3_256>), dim3(g), dim3(256), 0, c->stream, msgs, msg_stride, msg_len, out, n); break;
    case ECGPU_SHA3_384: hipLaunchKernelGGL((keccak_digest_kernel<keccak::Sha3_384>), dim3(g), dim3(256), 0, c->stream, msgs, msg_stride, msg_len, out, n); break;
    default: return ecgpu_set_err(c, ECGPU_ERR_ARG, "unknown hash %d", hash);
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}
