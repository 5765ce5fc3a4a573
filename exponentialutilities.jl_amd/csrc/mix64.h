// mix64.h -- the library's 64-bit mixer (the two-round multiply / xor-shift finaliser) and its salt: behind the content hash of
// expv_mi_host_wrapsum (capi.hip) and behind every "random" sign of the norm estimator (op_normest.hip), on the host and on the device.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace expv_mi {

__host__ __device__ inline uint64_t mix64(uint64_t h) {
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
  return h;
}
static constexpr uint64_t kHashSalt = 0x9e3779b97f4a7c15ull;

// The estimator's sign for natural row i of column `col` at draw `attempt`: +1 when the low bit of the mixed word is set, else -1.
__host__ __device__ inline int normest_sign(uint64_t i, uint32_t col, uint32_t attempt) {
  return (mix64(((i + 1) * kHashSalt) ^ (((uint64_t)col << 32) | (uint64_t)attempt)) & 1ull) ? 1 : -1;
}

}  // namespace expv_mi
