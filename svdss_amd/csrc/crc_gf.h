// crc_gf.h -- arithmetic of the CRC32 polynomial, shared by the CRC kernels of the BAM units (bam_device_internal.h) and of
// the plain-gzip unit (gzip_stream.hip): a lane's share of a CRC is a polynomial product.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// a(x) * b(x) mod P in the reflected representation zlib uses (bit 31 = x^0); P = 0xEDB88320
__host__ __device__ inline uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= (a & 0x80000000u) ? b : 0u;
    a <<= 1;
    b = (b >> 1) ^ ((b & 1u) ? 0xEDB88320u : 0u);
  }
  return p;
}
// x^(8 n) mod P
__host__ __device__ inline uint32_t gf_xpow8(uint32_t n) {
  uint32_t r = 0x80000000u;            // x^0
  uint32_t sq = 0x00800000u;           // x^8
  while (n) {
    if (n & 1u) r = gf_mul(r, sq);
    sq = gf_mul(sq, sq);
    n >>= 1;
  }
  return r;
}

}  // namespace
