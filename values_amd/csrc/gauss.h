// The Gaussian generator of the sampling kernels (accumulate.hip) and of the TTA noise views (noise.hip, tta2d.hip):
// Box-Muller on two avalanche hashes of (seed, stream b, element a).  Stream b of a seed is keyed by ONE word,
// seed ^ (b * 0x85EBCA6B + 0x165667B1); tests/sample_ref.py restates it in float64.
#pragma once
#include "common.h"

__device__ __forceinline__ float vx_gauss(uint32_t seed, uint32_t a, uint32_t b) {
  const uint32_t h1 = vx_mix32(a * 0x9E3779B1u ^ vx_mix32(seed ^ (b * 0x85EBCA6Bu + 0x165667B1u)));
  const uint32_t h2 = vx_mix32(h1 ^ 0x27D4EB2Fu ^ (a * 0xC2B2AE35u));
  const float u1 = ((float)(h1 >> 8) + 1.0f) * (1.0f / 16777216.0f);  // (0, 1]
  const float u2 = (float)(h2 >> 8) * (1.0f / 16777216.0f);           // [0, 1)
  return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

// The two hash words of vx_gauss by themselves, for a caller that wants uniforms (toydata.hip: (h >> 8) * 2^-24)
__device__ __forceinline__ void vx_gauss_words(uint32_t seed, uint32_t a, uint32_t b, uint32_t& h1, uint32_t& h2) {
  h1 = vx_mix32(a * 0x9E3779B1u ^ vx_mix32(seed ^ (b * 0x85EBCA6Bu + 0x165667B1u)));
  h2 = vx_mix32(h1 ^ 0x27D4EB2Fu ^ (a * 0xC2B2AE35u));
}

// The scale of a generated noise view: ONE uniform per stream b, the u2 word of element 0 of the streams of
// seed ^ VX_NOISE_SCALE_XOR -- no element stream of `seed` shares a key with them (the idiom of the SSN eps_w streams,
// seed ^ 0x5bd1e995, with a constant of its own).  var = lo + (hi - lo) * u2, u2 in [0, 1), two float32 roundings.
#define VX_NOISE_SCALE_XOR 0x3C6EF372u
__device__ __forceinline__ float vx_noise_var(uint32_t seed, uint32_t b, float lo, float hi) {
  const uint32_t h1 = vx_mix32(vx_mix32((seed ^ VX_NOISE_SCALE_XOR) ^ (b * 0x85EBCA6Bu + 0x165667B1u)));
  const uint32_t h2 = vx_mix32(h1 ^ 0x27D4EB2Fu);
  const float u2 = (float)(h2 >> 8) * (1.0f / 16777216.0f);           // [0, 1)
  return lo + (hi - lo) * u2;
}
// The scale itself, as vx_noise_view_3d (noise.hip) and vx_train_patches_3d (train_patches3d.hip) apply it to stream b:
// sigma_law 0: sqrt(var), 1: var
__device__ __forceinline__ float vx_noise_sigma(uint32_t seed, uint32_t b, float lo, float hi, int sigma_law) {
  const float var = vx_noise_var(seed, b, lo, hi);
  return sigma_law ? var : sqrtf(var);
}

// The label-switch decisions of the 2D test split (label_switch.hip): the h1 word of element r * n_switch + k of stream
// `image index` of seed ^ VX_LSWITCH_XOR -- the same idiom, a constant of its own: no stream is shared with the dropout,
// SSN or noise draws of the same seed.
#define VX_LSWITCH_XOR 0xA54FF53Au
