// The colour -> train id lookup of color2trainId.get(tuple(x), default): shared by rgb_to_trainid_kernel (png_decode.hip)
// and crop_resize_kernel (preprocess2d.hip).  The table is n <= RT_MAX pairs (0x00RRGGBB key, id) of uint32, staged in
// LDS once per workgroup and scanned in order, so of two entries with one key the later one counts.
#pragma once
#include <stdint.h>

constexpr int RT_MAX = 256;

// every thread of the workgroup calls it; ends with a workgroup barrier
template <int THREADS>
__device__ __forceinline__ void rt_stage(const uint32_t* __restrict__ table, int n_table, uint32_t* key, uint32_t* id) {
  for (int j = threadIdx.x; j < n_table; j += THREADS) {
    key[j] = table[2 * j] & 0xFFFFFFu;
    id[j] = table[2 * j + 1] & 0xFFu;
  }
  __syncthreads();
}

// r[k] = the id of px[k]'s entry; r comes in holding the default
template <int N>
__device__ __forceinline__ void rt_lookup(const uint32_t* key, const uint32_t* id, int n_table, const uint32_t (&px)[N], uint32_t (&r)[N]) {
  for (int j = 0; j < n_table; ++j) {
    const uint32_t kj = key[j], ij = id[j];
#pragma unroll
    for (int k = 0; k < N; ++k) r[k] = px[k] == kj ? ij : r[k];
  }
}
