// A whole batch of the 3D train / validation loaders in one launch (values_amd.datamodule3d.DeviceLoader3D):
// per item the crop of NumpyDataLoader, MirrorTransform, GaussianNoiseTransform and the float cast of NumpyToTensor, from
// resident file payloads of different cases, shapes and stored dtypes, for the image and the drawn rater's label in the
// same pass.  HBM-bound without noise; with noise the generator's arithmetic bounds it, as it bounds noise.hip.
// Lanes run along z, four consecutive z per lane (vx4_access.h decides per access: one of up to 16 bytes where the four
// elements lie inside the row and the address is aligned to it, element by element elsewhere).  A z-mirror loads FORWARD
// from the mirrored source address and reverses the elements in registers.  Plain C++ loads and stores; the only atomic is
// the integer count of labels outside 0..255.  No byte outside a crop or an output array is touched.
// The reference adds its noise in float64 before the cast to float32; this kernel adds it in float32 after the cast (one
// fmaf, the expression of noise.hip: bit-equal to vx_noise_view_3d over the noise-free patch).
// train3d_plan.h holds every argument check and the lane -> (output row, source run) decomposition; the item table goes up
// through the pinned staging buffer of staging.h: no wait on the stream, not capturable into a hipGraph.
#include "common.h"
#include "gauss.h"
#include "staging.h"
#include "train3d_plan.h"
#include "vx4_access.h"

struct T3Seed { const uint32_t* seed_dev; };   // (the argument shape vx_seed_of reads)

// v[0 .. n) reversed in place, n in 1..4, with constant register indices only
template <typename S>
__device__ __forceinline__ void t3_reverse(S v[4], int n) {
  const int hi = n - 1;
  S t;
  if (hi == 3) { t = v[0]; v[0] = v[3]; v[3] = t; t = v[1]; v[1] = v[2]; v[2] = t; }
  else if (hi == 2) { t = v[0]; v[0] = v[2]; v[2] = t; }
  else if (hi == 1) { t = v[0]; v[0] = v[1]; v[1] = t; }
}

__global__ __launch_bounds__(T3_THREADS) void train_patches_3d_kernel(const t3_item* __restrict__ items, int n_items, t3_shape sh,
                                                                      float* __restrict__ data, void* __restrict__ seg, int seg_u8,
                                                                      uint32_t seed, T3Seed sd, float lo, float hi, int sigma_law,
                                                                      float* __restrict__ sigma_out, int32_t* __restrict__ status) {
  const uint32_t s = vx_seed_of(sd, seed);
  const int64_t total = (int64_t)n_items * sh.per;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int it = (int)(i / sh.per);
    const t3_item g = items[it];
    const t3_lane l = t3_lane_of(sh, i - (int64_t)it * sh.per, g.D1, g.D2, g.o0, g.o1, g.o2, g.flags);
    double d[4];
    vx4_load_kind(g.image, g.kind, l.src, l.n, d);
    if (l.rev) t3_reverse(d, l.n);
    float f[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) f[u] = (float)d[u];   // round to nearest even, as astype(float32)
    const bool noisy = (g.flags & VX_TRAIN3D_NOISE) != 0;
    float sg = 0.f;
    if (noisy) {
      sg = vx_noise_sigma(s, g.index, lo, hi, sigma_law);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (u < l.n) f[u] = fmaf(sg, vx_gauss(s, (uint32_t)(l.dst + u), g.index), f[u]);
    }
    if (sigma_out && l.dst == 0) sigma_out[it] = sg;
    const int64_t o = (int64_t)it * sh.pv + l.dst;
    vx4_store<float>(data + o, l.n, f);
    if (seg) {
      int32_t lab[4] = {0, 0, 0, 0};
      if (g.label) {
        bool bad[4];
        vx4_load_label(g.label, g.esl, g.sgn, l.src, l.n, lab, bad);
        int nbad = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) nbad += bad[u] ? 1 : 0;
        if (nbad) atomicAdd(&status[it], nbad);   // a lane's neighbours may belong to other items: no wave reduction
        if (l.rev) t3_reverse(lab, l.n);
      }
      if (seg_u8) {
        uint8_t b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) b[u] = (uint8_t)lab[u];
        vx4_store<uint8_t>(reinterpret_cast<uint8_t*>(seg) + o, l.n, b);
      } else {
        float q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = (float)lab[u];
        vx4_store<float>(reinterpret_cast<float*>(seg) + o, l.n, q);
      }
    }
  }
}

static vx_staging g_train3d_stage;

extern "C" int64_t vx_train_patches_3d_workspace_bytes(int n_items) { return t3_workspace_bytes(n_items); }

extern "C" int vx_train_patches_3d(const vx_train3d_item* items, int n_items, int P0, int P1, int P2, float* data, void* seg, int seg_u8,
                                   uint32_t seed, const uint32_t* seed_dev, float var_lo, float var_hi, int sigma_law, float* sigma_out,
                                   int32_t* status, void* workspace, int64_t ws_bytes, vx_stream_t stream) {
  const char* who = "vx_train_patches_3d";
  t3_plan p;
  const int rc = t3_make_plan(items, n_items, P0, P1, P2, data, seg, seg_u8, var_lo, var_hi, sigma_law, sigma_out, status, workspace,
                              ws_bytes, &p);
  if (rc != VX_OK) VX_FAIL(rc, "%s", p.err);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(status, 0, (size_t)n_items * sizeof(int32_t), s);
  if (e != hipSuccess) VX_FAIL((int)e, "%s: memset: %s", who, hipGetErrorString(e));
  const vx_stage_part part = {p.table.data(), p.table.size() * sizeof(t3_item), 0};
  const int up = vx_staged_upload(g_train3d_stage, who, &part, 1, part.bytes, workspace, s);
  if (up != VX_OK) return up;
  T3Seed sd = {seed_dev};
  hipLaunchKernelGGL(train_patches_3d_kernel, dim3(p.grid), dim3(T3_THREADS), 0, s, (const t3_item*)workspace, n_items, p.shape, data, seg,
                     seg_u8, seed, sd, var_lo, var_hi, sigma_law, sigma_out, status);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}
