// The TTA branch of Cityscapes_dataset.__getitem__ (uncertainty_modeling/data/cityscapes_dataset.py:76-99) on the device:
// one launch turns a batch of images into the G normalised views the 2D driver forwards (test_2D.py:299-311), already in
// the layout the stem convolution stages from -- channels-last float32 at pitch 4 (channel 3 = 0) -- with the flips as index
// arithmetic.  The host path (values_amd.data.tta_views_2d + torch.flip / permute / zero-fill per view) moved 6 tensors
// per view through ATen kernels; this is one streaming pass: 3 (+12) bytes read, 16 bytes written per output pixel.
//
//   u8 source (the reference's dataset path): img [B][H][W][3] uint8; a noisy view adds a float field to the uint8 image,
//     clips to 0..255 and truncates back to uint8 (albumentations.GaussNoise on uint8 input) BEFORE
//     Normalize(mean, std, max_pixel_value) = (v - mean * max) * (1 / (std * max)), evaluated as values_amd.data.tta_views_2d
//     does (two float32 roundings): bit-exact with it.  The noise field of a flipped view is indexed in the VIEW's
//     coordinates (the dataset applies GaussNoise after HorizontalFlip: an independent draw per view) unless the view code
//     says otherwise (bit 3: the field travels with the image -- "flip of the noisy image", the 8-view set of config C4).
//   f32 source (already normalised tensors, what values_amd.predict2d.tta_views_8 takes): clean / noisy [B][3][H][W].
//
// vx_tta_views_2d_gen (view-code bit 5): the additive field of a noisy view is DRAWN here instead of read --
//     sqrt(var_{b,k}) * vx_gauss(seed', (y * W + x) * 3 + c, (image0 + b) * 2 + k),   var_{b,k} ~ U(var_limit)
// (albumentations' GaussNoise(var_limit, mean=0, per_channel=True) as a distribution; the stream is this project's), which
// takes the two float32 fields -- 12 of the 15 input bytes per pixel -- out of the pass: 3 bytes read, 16 written.  Both
// entries launch the one kernel body below; a call without a generated view runs the instance without the generator.
#include "common.h"
#include "gauss.h"

namespace {
struct TtaArgs {
  const void* src;          // u8 [B][H][W][3]  |  f32 [B][3][H][W]
  const float* noise[2];    // u8: additive fields [B][H][W][3] (slot 0 / 1, nullable);  f32: noise[0] = the noisy tensor [B][3][H][W]
  float mean255[3], inv[3];
  float* out;               // [G][B][H][W][4]
  int B, H, W, G;
  int code[16];             // per view: bit 0 hflip, bit 1 vflip, bit 2 noisy, bit 3 field indexed at the SOURCE pixel, bit 4 noise slot,
                            // bit 5 the field is generated (u8 source)
  uint32_t seed, image0;    // generated fields: stream (image0 + b) * 2 + slot of seed + *seed_dev
  const uint32_t* seed_dev;
  float var_lo, var_hi;
  float* sigma_out;         // [B][2], nullable
};

template <bool U8, bool GEN>
__global__ __launch_bounds__(256) void tta_views_2d_kernel(TtaArgs a) {
  const int64_t per = (int64_t)a.H * a.W;
  const int64_t total = per * a.B * a.G;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % a.W);
    int64_t r = i / a.W;
    const int y = (int)(r % a.H); r /= a.H;
    const int b = (int)(r % a.B);
    const int g = (int)(r / a.B);
    const int code = a.code[g];
    const int xs = (code & 1) ? a.W - 1 - x : x;
    const int ys = (code & 2) ? a.H - 1 - y : y;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if constexpr (U8) {
      const uint8_t* p = reinterpret_cast<const uint8_t*>(a.src) + ((int64_t)b * per + (int64_t)ys * a.W + xs) * 3;
      const float* nf = (code & 4) ? a.noise[(code >> 4) & 1] : nullptr;
      const int64_t ni = (code & 8) ? ((int64_t)b * per + (int64_t)ys * a.W + xs) * 3 : ((int64_t)b * per + (int64_t)y * a.W + x) * 3;
      bool gen = false;
      uint32_t gs = 0, slot = 0, e0 = 0;
      float sg = 0.f;
      if constexpr (GEN) {
        gs = vx_seed_of(a, a.seed);
        if (a.sigma_out && g == 0 && x == 0 && y == 0) {       // both slots of the image, whichever views use them
          a.sigma_out[b * 2 + 0] = sqrtf(vx_noise_var(gs, (a.image0 + (uint32_t)b) * 2u, a.var_lo, a.var_hi));
          a.sigma_out[b * 2 + 1] = sqrtf(vx_noise_var(gs, (a.image0 + (uint32_t)b) * 2u + 1u, a.var_lo, a.var_hi));
        }
        gen = (code & 32) != 0;
        if (gen) {
          nf = nullptr;
          slot = (a.image0 + (uint32_t)b) * 2u + (uint32_t)((code >> 4) & 1);
          sg = sqrtf(vx_noise_var(gs, slot, a.var_lo, a.var_hi));
          e0 = (uint32_t)(ni - (int64_t)b * per * 3);            // (y * W + x) * 3 in the field's coordinates
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float v = (float)p[c];
        if (nf || (GEN && gen)) {
          const float n = (GEN && gen) ? sg * vx_gauss(gs, e0 + (uint32_t)c, slot) : nf[ni + c];
          v = fminf(fmaxf(v + n, 0.f), 255.f);              // np.clip(img.astype(float32) + n, 0, 255)
          v = (float)(uint8_t)v;                            // .astype(uint8): truncation
        }
        o[c] = (v - a.mean255[c]) * a.inv[c];
      }
    } else {
      const float* base = (code & 4) ? a.noise[0] : reinterpret_cast<const float*>(a.src);
      const float* p = base + (int64_t)b * 3 * per + (int64_t)ys * a.W + xs;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = p[(int64_t)c * per];
    }
    *reinterpret_cast<f32x4*>(a.out + i * 4) = o;
  }
}
}  // namespace

static int tta_launch(const char* who, int max_code, const void* src, int src_u8, const float* noise0, const float* noise1,
                      const float* mean, const float* std, float max_pixel_value, int B, int H, int W, int G,
                      const int32_t* view_code, uint32_t seed, const uint32_t* seed_dev, int64_t image0, const float* var_limit,
                      float* sigma_out, float* out, vx_stream_t stream) {
  if (!src || !out || !view_code) VX_FAIL(VX_E_NULL, "%s: null pointer", who);
  if (B <= 0 || H <= 0 || W <= 0 || G <= 0 || G > 16) VX_FAIL(VX_E_SHAPE, "%s: B=%d H=%d W=%d G=%d (1..16 views)", who, B, H, W, G);
  if (!vx_aligned16(out)) VX_FAIL(VX_E_ALIGN, "%s: out must be 16-byte aligned", who);
  TtaArgs a = {};
  a.src = src; a.noise[0] = noise0; a.noise[1] = noise1; a.out = out;
  a.B = B; a.H = H; a.W = W; a.G = G;
  bool gen = false;
  for (int g = 0; g < G; ++g) {
    const int c = view_code[g];      // HOST array: the view list is part of the call, like the transform names of the dataset
    if (c < 0 || c > max_code) VX_FAIL(VX_E_DTYPE, "%s: view code %d", who, c);
    if (c & 32) {
      if (!src_u8) VX_FAIL(VX_E_DTYPE, "%s: view %d: generated noise is defined for the uint8 source only", who, g);
      if (!(c & 4)) VX_FAIL(VX_E_DTYPE, "%s: view code %d: bit 5 (generated) without bit 2 (noisy)", who, c);
      gen = true;
    } else if ((c & 4) && !a.noise[src_u8 ? (c >> 4) & 1 : 0]) {
      VX_FAIL(VX_E_NULL, "%s: view %d is noisy but its noise tensor is null", who, g);
    }
    a.code[g] = c;
  }
  if (src_u8) {
    if (!mean || !std || !(max_pixel_value > 0.f)) VX_FAIL(VX_E_NULL, "%s: uint8 source needs mean / std / max_pixel_value", who);
    for (int c = 0; c < 3; ++c) {
      a.mean255[c] = mean[c] * max_pixel_value;            // float32 products, as numpy forms them
      a.inv[c] = 1.0f / (std[c] * max_pixel_value);
    }
  }
  if (gen) {
    if (!var_limit) VX_FAIL(VX_E_NULL, "%s: generated views need var_limit", who);
    if (!(var_limit[0] >= 0.f) || !(var_limit[1] >= var_limit[0]) || !(var_limit[1] < INFINITY))
      VX_FAIL(VX_E_SHAPE, "%s: var_limit (%g, %g)", who, var_limit[0], var_limit[1]);
    if ((int64_t)H * W * 3 >= (1ll << 32)) VX_FAIL(VX_E_SHAPE, "%s: image too large for a generated field", who);
    if (image0 < 0 || (image0 + B) * 2 > (1ll << 32)) VX_FAIL(VX_E_SHAPE, "%s: (image0 + B) * 2 must fit 32 bits", who);
    a.seed = seed; a.seed_dev = seed_dev; a.image0 = (uint32_t)image0;
    a.var_lo = var_limit[0]; a.var_hi = var_limit[1];
    a.sigma_out = sigma_out;
  }
  const int64_t total = (int64_t)G * B * H * W;
  int bx = (int)((total + 255) / 256);
  if (bx > 16384) bx = 16384;
  if (gen) hipLaunchKernelGGL((tta_views_2d_kernel<true, true>), dim3((unsigned)bx), dim3(256), 0, (hipStream_t)stream, a);
  else if (src_u8) hipLaunchKernelGGL((tta_views_2d_kernel<true, false>), dim3((unsigned)bx), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((tta_views_2d_kernel<false, false>), dim3((unsigned)bx), dim3(256), 0, (hipStream_t)stream, a);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}

extern "C" int vx_tta_views_2d(const void* src, int src_u8, const float* noise0, const float* noise1, const float* mean,
                               const float* std, float max_pixel_value, int B, int H, int W, int G, const int32_t* view_code,
                               float* out, vx_stream_t stream) {
  return tta_launch("vx_tta_views_2d", 31, src, src_u8, noise0, noise1, mean, std, max_pixel_value, B, H, W, G, view_code, 0,
                    nullptr, 0, nullptr, nullptr, out, stream);
}

extern "C" int vx_tta_views_2d_gen(const void* src, int src_u8, const float* noise0, const float* noise1, const float* mean,
                                   const float* std, float max_pixel_value, int B, int H, int W, int G,
                                   const int32_t* view_code, uint32_t seed, const uint32_t* seed_dev, int64_t image0,
                                   const float* var_limit, float* sigma_out, float* out, vx_stream_t stream) {
  return tta_launch("vx_tta_views_2d_gen", 63, src, src_u8, noise0, noise1, mean, std, max_pixel_value, B, H, W, G, view_code,
                    seed, seed_dev, image0, var_limit, sigma_out, out, stream);
}
