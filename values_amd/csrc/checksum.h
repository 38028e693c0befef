// Checksums of the DEFLATE containers, shared by the encoders (deflate_chunk.hip, gzip.hip, png.hip) and the decoder
// (inflate.hip): CRC-32 (gzip members, PNG chunks) with its GF(2) shift and join operators, and the Adler-32 join (zlib
// streams).  Internal linkage: each including file compiles its own copy.
#pragma once
#include "common.h"

namespace {

constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr uint32_t ADLER_BASE = 65521u;

__host__ __device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

struct CrcTables {
  uint32_t byte[256];
  uint32_t x2n[32];   // x^(2^k) mod P, reflected
};

constexpr uint32_t crc_multmodp_c(uint32_t a, uint32_t b) {
  uint32_t m = 1u << 31, p = 0;
  for (;;) {
    if (a & m) {
      p ^= b;
      if ((a & (m - 1)) == 0) break;
    }
    m >>= 1;
    b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
  }
  return p;
}

constexpr CrcTables make_crc_tables() {
  CrcTables t{};
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ CRC_POLY : c >> 1;
    t.byte[i] = c;
  }
  uint32_t p = 1u << 30;   // x^1
  t.x2n[0] = p;
  for (int n = 1; n < 32; ++n) t.x2n[n] = p = crc_multmodp_c(p, p);
  return t;
}

__constant__ CrcTables kCrc = make_crc_tables();

__device__ uint32_t crc_multmodp(uint32_t a, uint32_t b) {
  uint32_t m = 1u << 31, p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & m) p ^= b;
    m >>= 1;
    b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
  }
  return p;
}
// x^(8 n) mod P: the operator that shifts a CRC over n zero bytes
__device__ uint32_t crc_shift_op(uint64_t n) {
  uint32_t p = 1u << 31;
  int k = 3;
  while (n) {
    if (n & 1) p = crc_multmodp(kCrc.x2n[k & 31], p);
    n >>= 1;
    ++k;
  }
  return p;
}
// crc32(A || B) from crc32(A), crc32(B) and |B|
__device__ uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  return len_b ? crc_multmodp(crc_shift_op(len_b), crc_a) ^ crc_b : crc_a;
}

// tree join of the per-lane CRCs of consecutive slices (crc[], len[] in LDS; all lanes of the block call it)
template <int N>
__device__ void crc_join_block(uint32_t* crc, uint32_t* len) {
  const int l = threadIdx.x;
  for (int stride = 1; stride < N; stride <<= 1) {
    __syncthreads();
    if ((l % (2 * stride)) == 0 && l + stride < N) {
      crc[l] = crc_combine(crc[l], crc[l + stride], len[l + stride]);
      len[l] += len[l + stride];
    }
  }
  __syncthreads();
}

__device__ __forceinline__ uint32_t adler_combine(uint32_t a1, uint32_t a2, uint64_t len2) {
  // adler32(A || B): s1 = s1A + s1B - 1, s2 = s2A + s2B + |B| (s1A - 1), mod 65521 (zlib's adler32_combine)
  const uint64_t B = ADLER_BASE;
  const uint64_t s1a = a1 & 0xFFFFu, s2a = a1 >> 16, s1b = a2 & 0xFFFFu, s2b = a2 >> 16;
  const uint64_t r = len2 % B;
  const uint64_t s1 = (s1a + s1b + B - 1) % B;
  const uint64_t s2 = (s2a + s2b + r * ((s1a + B - 1) % B)) % B;
  return (uint32_t)((s2 << 16) | s1);
}

}  // namespace
