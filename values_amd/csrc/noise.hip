// The noisy TTA input of predict_cases (test_3D.py:428: batchgenerators' GaussianNoiseTransform, variance ~ U(0, 0.1)) drawn
// on the device from a seed:
//     out[v][r] = x[v][r] + sigma_g * vx_gauss(seed', r, g),   g = index0 + v,   seed' = seed + *seed_dev
// The stream of a volume is keyed by the seed and the volume's GLOBAL index g alone, so the view does not depend on how
// the caller chunks, shards or batches; sigma_g follows from one uniform of a stream no element shares (vx_noise_var,
// gauss.h).  The DISTRIBUTION is the reference's, the stream is this project's (the reference draws from numpy's global
// generator inside a third-party transform: bit parity is out of reach).  One grid-stride streaming pass, 4 B read and
// 4 B written per element, no LDS, no matrix cores; measured, the generator's arithmetic bounds it, not HBM.
#include "common.h"
#include "gauss.h"

struct NoiseSeed { const uint32_t* seed_dev; };   // (the argument shape vx_seed_of reads)

__global__ __launch_bounds__(256) void noise_view_3d_kernel(const float* x, float* out, int V, int64_t per, uint32_t seed,
                                                            NoiseSeed sd, uint32_t index0, float lo, float hi, int sigma_law,
                                                            float* __restrict__ sigma_out) {
  const uint32_t s = vx_seed_of(sd, seed);
  const int64_t total = (int64_t)V * per;
  int last = -1;
  float sg = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int v = (int)(i / per);
    const int64_t r = i - (int64_t)v * per;
    if (v != last) {            // one scale per volume: a thread meets a new volume once per `per` elements of its stride
      sg = vx_noise_sigma(s, index0 + (uint32_t)v, lo, hi, sigma_law);
      last = v;
    }
    if (sigma_out && r == 0) sigma_out[v] = sg;
    out[i] = fmaf(sg, vx_gauss(s, (uint32_t)r, index0 + (uint32_t)v), x[i]);
  }
}

extern "C" int vx_noise_view_3d(const float* x, float* out, int V, int64_t per, uint32_t seed, const uint32_t* seed_dev,
                                int64_t index0, float var_lo, float var_hi, int sigma_law, float* sigma_out,
                                vx_stream_t stream) {
  if (V <= 0 || per < 0) VX_FAIL(VX_E_SHAPE, "vx_noise_view_3d: bad shape");
  if (per >= (1ll << 32)) VX_FAIL(VX_E_SHAPE, "vx_noise_view_3d: volume too large");
  if (index0 < 0 || index0 + V > (1ll << 32)) VX_FAIL(VX_E_SHAPE, "vx_noise_view_3d: index0 + V must fit 32 bits");
  if (!(var_lo >= 0.f)) VX_FAIL(VX_E_SHAPE, "vx_noise_view_3d: variance range starts below 0");
  if (!(var_hi >= var_lo) || !(var_hi < INFINITY)) VX_FAIL(VX_E_SHAPE, "vx_noise_view_3d: variance range (%g, %g)", var_lo, var_hi);
  if (sigma_law != 0 && sigma_law != 1) VX_FAIL(VX_E_DTYPE, "vx_noise_view_3d: sigma_law %d (0: sqrt(var), 1: var)", sigma_law);
  if (per == 0) return VX_OK;
  if (!x || !out) VX_FAIL(VX_E_NULL, "vx_noise_view_3d: null pointer");
  const int64_t total = (int64_t)V * per;
  const int64_t nb = (total + 255) / 256;
  const int bx = nb > 16384 ? 16384 : (int)nb;       // the launch shape of vx_aleatoric_sample
  NoiseSeed sd = {seed_dev};
  hipLaunchKernelGGL(noise_view_3d_kernel, dim3(bx), dim3(256), 0, (hipStream_t)stream, x, out, V, per, seed, sd,
                     (uint32_t)index0, var_lo, var_hi, sigma_law, sigma_out);
  VX_CHECK_LAUNCH("vx_noise_view_3d");
  return VX_OK;
}
