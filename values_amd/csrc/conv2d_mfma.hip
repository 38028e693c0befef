// K15: 2D convolutions of HRNet (uncertainty_modeling/models/hrnet_module.py:37-41, 85-93, 349-358, 411-428):
// 3x3 stride 1, 3x3 stride 2, 1x1 -- channels-last fp32, implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32),
// same skeleton as conv3d_mfma.hip: persistent 512-thread workgroups over a flat list of (tile, cin-chunk) items,
// next item's loads in flight in registers (buffer loads, out-of-image pieces steered out of range -> zeros),
// group-major conflict-free LDS image, weights pre-packed in fragment order.
//
//   D[cout][x] = sum_k W[cout][k] X[k][x],  k = (ky, kx, cin);  rows = 16*NT couts, columns = 16 consecutive output x
//   Workgroup tile = 16 (x) x TY (y) outputs; wave w owns R = TY/8 rows.
//   Stride 2: output x reads input 2x + kx - 1, so even/odd input columns (and rows) live in separate parity planes
//   of the LDS image and a tile's 16 columns stay consecutive positions (same trick as the 3D x-pair packing).
//   1x1: no halo, up to NSUB = 4 sub-blocks of 16 input channels per item (a GEMM with K = 64 per barrier pair).
//
// Epilogue: optional bias, raw store, and per-workgroup (sum, sum of squares) partials per channel for the
// TRAINING-mode BatchNorm that follows every conv (batch statistics over N,H,W) -- deterministic, no
// atomics; vx_bn_finalize reduces them.
#include "conv2d_internal.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct Conv2dKArgs {
  vx_conv2d_args a;
  int OH, OW, tiles_x, tiles_y, nchunks;   // Conv2dRoute's (nchunks = ceil(Cin/16 / NSUB))
  unsigned mx, my;
};

namespace {
constexpr unsigned K_OOB = 0xFFFFFFF0u;
constexpr unsigned K_NUMREC = 0x80000000u;
}

template <int KS, int S, int NT, int NSUB, int TY>
__global__ __launch_bounds__(512) void conv2d_mfma_kernel(Conv2dKArgs ka) {
  constexpr int NW = 8, NTH = 512, TX = 16;
  constexpr int R = TY / NW;
  // the instance's LDS layout (conv2d_route.h, where the launch geometry reads the same numbers)
  constexpr C2Geo G = c2_geo(KS, S, NT, NSUB, TY);
  constexpr int HX = G.t.HX, HY = G.t.HY, PXW = G.t.PXW, NPP = G.t.NPP, PLANE = G.t.PLANE;
  constexpr int IN_FLOATS = G.IN_FLOATS, NTAP = KS * KS, W_SUB = G.W_SUB, W_FLOATS = G.W_FLOATS;
  constexpr int NPIECE = HX * HY * 4 * NSUB;                      // 16-byte pieces of the input tile
  constexpr int IN_IT = (NPIECE + NTH - 1) / NTH;
  constexpr int W_IT = (W_FLOATS / 4 + NTH - 1) / NTH;
  static_assert(TY % NW == 0 && IN_IT <= 16, "tile config");

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* s_in = smem;
  float* s_w = smem + IN_FLOATS;

  const vx_conv2d_args& a = ka.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, g = lane >> 4;
  const int cg = blockIdx.y;
  const int ntiles = ka.tiles_x * ka.tiles_y;
  const int total = ntiles * a.N;
  const int lastx = (ka.tiles_x - 1) * TX, lasty = (ka.tiles_y - 1) * TY;  // output coords of the last tile
  const int nsub_all = a.Cin / 16;

  // ---- per-lane constants ----
  int vbase[R];
  unsigned ovoff[R];
  unsigned obad_xhi = 0, obad_yhi = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int ly = wave * R + r;
    vbase[r] = (g * PLANE + ly * PXW + m) * 4;
    ovoff[r] = (unsigned)(((ly * ka.OW + m) * a.out_pitch + a.out_coff + g * 4) * 4);
    if (m >= ka.OW - lastx) obad_xhi |= 1u << r;
    if (ly >= ka.OH - lasty) obad_yhi |= 1u << r;
  }
  // staging pattern: piece idx -> (sub, hy, hx, q)
  const int rowf = a.W * a.in_pitch;
  const int biasf = KS == 1 ? 0 : rowf + a.in_pitch;   // one row + one pixel of padding offset
  unsigned voff[IN_IT];
  int ldst[IN_IT];
  unsigned ibad_always = 0, ibad_xlo = 0, ibad_xhi = 0, ibad_ylo = 0, ibad_yhi = 0;
  unsigned isub[IN_IT];
#pragma unroll
  for (int it = 0; it < IN_IT; ++it) {
    const int idx = tid + it * NTH;
    const int q = idx % 4;
    const int pix = (idx / 4) % (HX * HY);
    const int sub = idx / (4 * HX * HY);
    const int hx = pix % HX, hy = pix / HX;
    const int dxr = hx - KS / 2, dyr = hy - KS / 2;       // input pixel relative to the tile's input origin
    voff[it] = (unsigned)((dyr * rowf + dxr * a.in_pitch + sub * 16 + q * 4 + biasf) * 4);
    const int par = (hy % S) * S + (hx % S);
    ldst[it] = ((sub * 4 + q) * PLANE + par * NPP + (hy / S) * PXW + hx / S) * 4;
    isub[it] = (unsigned)sub;
    if (idx >= NPIECE) ibad_always |= 1u << it;
    if (dxr < 0) ibad_xlo |= 1u << it;
    if (dxr >= a.W - lastx * S) ibad_xhi |= 1u << it;
    if (dyr < 0) ibad_ylo |= 1u << it;
    if (dyr >= a.H - lasty * S) ibad_yhi |= 1u << it;
  }
  const size_t in_sample = (size_t)a.H * rowf;
  const size_t out_sample = (size_t)ka.OH * ka.OW * a.out_pitch;

  auto decode = [&](int t_, int& n, int& tx, int& ty) {
    unsigned t = (unsigned)t_, q;
    q = ka.tiles_x == 1 ? t : __umulhi(t, ka.mx); tx = (int)(t - q * ka.tiles_x); t = q;
    q = ka.tiles_y == 1 ? t : __umulhi(t, ka.my); ty = (int)(t - q * ka.tiles_y); n = (int)q;
  };

  const float* w_cg = a.w_packed + (size_t)cg * nsub_all * W_SUB;
  f32x4 ibuf[IN_IT], wbuf[W_IT];
  const bool w_resident = ka.nchunks == 1;
  bool w_fresh = true;

  auto prefetch = [&](int tile_lin, int chunk, bool have, bool with_w) {
    int n, tx, ty;
    decode(tile_lin, n, tx, ty);
    const int nsub = min(NSUB, nsub_all - chunk * NSUB);   // sub-blocks in this chunk
    unsigned bad = ibad_always;
    if (tx == 0) bad |= ibad_xlo;
    if (tx == ka.tiles_x - 1) bad |= ibad_xhi;
    if (ty == 0) bad |= ibad_ylo;
    if (ty == ka.tiles_y - 1) bad |= ibad_yhi;
    if (!have) bad = 0xFFFFFFFFu;
    const unsigned soff = (unsigned)(((ty * TY * S) * rowf + (tx * TX * S) * a.in_pitch + chunk * NSUB * 16) * 4);
    const __amdgpu_buffer_rsrc_t srd = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.in + (size_t)(have ? n : 0) * in_sample - biasf), 0, K_NUMREC, 0x00020000);
    // channels at and beyond min(Cin, in_pitch) read as zero: a tensor of C real channels may arrive with pitch round4(C)
    // (HRNet-W18's 18-channel branch: 20 floats per pixel instead of 32)
    const int clim = min(a.Cin, a.in_pitch) - chunk * NSUB * 16;
#pragma unroll
    for (int it = 0; it < IN_IT; ++it) {
      const bool b = ((bad >> it) & 1u) || (int)isub[it] * 16 + (tid & 3) * 4 >= clim;   // NTH % 4 == 0: q = tid % 4
      const unsigned vo = b ? K_OOB : voff[it];
      ibuf[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd, (int)vo, (int)soff, 0));
    }
    const f32x4* src = reinterpret_cast<const f32x4*>(w_cg + (size_t)chunk * NSUB * W_SUB);
#pragma unroll
    for (int it = 0; it < W_IT; ++it) {
      const int idx = tid + it * NTH;
      f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (have && with_w && idx < nsub * (W_SUB / 4)) v = src[idx];
      wbuf[it] = v;
    }
  };
  auto commit = [&](bool with_w) {
#pragma unroll
    for (int it = 0; it < IN_IT; ++it)
      if (tid + it * NTH < NPIECE) *reinterpret_cast<f32x4*>(s_in + ldst[it]) = ibuf[it];
    if (with_w) {
#pragma unroll
      for (int it = 0; it < W_IT; ++it) {
        const int idx = tid + it * NTH;
        if (idx < W_FLOATS / 4) reinterpret_cast<f32x4*>(s_w)[idx] = wbuf[it];
      }
    }
  };

  f32x4 bias4[NT];
  bool cvalid[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int co = (cg * NT + nt) * 16 + g * 4;
    cvalid[nt] = co < a.Cout;
    bias4[nt] = (a.bias && cvalid[nt]) ? *reinterpret_cast<const f32x4*>(a.bias + co) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  int tile_lin = blockIdx.x, chunk = 0;
  bool have = tile_lin < total;
  prefetch(tile_lin, 0, have, true);
  f32x4 acc[R][NT];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[r][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  while (have) {
    __syncthreads();
    commit(w_fresh);
    __syncthreads();
    w_fresh = !w_resident;
    const int nsub = min(NSUB, nsub_all - chunk * NSUB);
    int ntile = tile_lin, nchunk = chunk + 1;
    if (nchunk == ka.nchunks) { nchunk = 0; ntile = tile_lin + (int)gridDim.x; }
    const bool nhave = ntile < total;
    prefetch(ntile, nchunk, nhave, !w_resident);

    for (int sub = 0; sub < nsub; ++sub) {   // NSUB == 1: a single pass
      const float* sw = s_w + sub * W_SUB;
      const float* si = s_in + sub * 4 * PLANE * 4;
      f32x4 wf[2][NT], xf[2][R];
      auto load_tap = [&](int t1, int slot) {
        const int ky = t1 / KS, kx = t1 % KS;
        const int toff = (((ky % S) * S + (kx % S)) * NPP + (ky / S) * PXW + kx / S) * 4;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wf[slot][nt] = *reinterpret_cast<const f32x4*>(sw + ((t1 * NT + nt) * 64 + lane) * 4);
#pragma unroll
        for (int r = 0; r < R; ++r) xf[slot][r] = *reinterpret_cast<const f32x4*>(si + vbase[r] + toff);
      };
      load_tap(0, 0);
#pragma unroll
      for (int tap = 0; tap < NTAP; ++tap) {
        if (tap + 1 < NTAP) load_tap(tap + 1, (tap + 1) & 1);
        const int cur = tap & 1;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[cur][nt][j], xf[cur][r][j], acc[r][nt], 0, 0, 0);
      }
    }

    if (chunk == ka.nchunks - 1) {
      int n, tx, ty;
      decode(tile_lin, n, tx, ty);
      unsigned obad = 0;
      if (tx == ka.tiles_x - 1) obad |= obad_xhi;
      if (ty == ka.tiles_y - 1) obad |= obad_yhi;
      const unsigned osoff = (unsigned)((ty * TY * ka.OW + tx * TX) * a.out_pitch) * 4u;
      const __amdgpu_buffer_rsrc_t osrd =
          __builtin_amdgcn_make_buffer_rsrc((void*)(a.out + (size_t)n * out_sample), 0, K_NUMREC, 0x00020000);
      float ssum[NT][4], ssq[NT][4];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j) { ssum[nt][j] = 0.f; ssq[nt][j] = 0.f; }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const unsigned cshift = (unsigned)((cg * NT + nt) * 16);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const bool bad = ((obad >> r) & 1u) || !cvalid[nt];
          const f32x4 v = acc[r][nt] + bias4[nt];
          if (a.stats_partial && !bad) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { ssum[nt][j] += v[j]; ssq[nt][j] += v[j] * v[j]; }
          }
          const unsigned vo = bad ? K_OOB : ovoff[r] + cshift * 4u;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), osrd, (int)vo, (int)osoff, 0);
          // gfx950 store-data hazard with an SGPR soffset (see conv3d_mfma.hip)
          __builtin_amdgcn_sched_barrier(0);
          asm volatile("s_nop 3" ::: "memory");
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (a.stats_partial) {
        float* s_red = smem + IN_FLOATS + W_FLOATS;  // [NW][NT][16][2]
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float s = ssum[nt][j], q = ssq[nt][j];
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) { s += __shfl_xor(s, off, 64); q += __shfl_xor(q, off, 64); }
            if (m == 0) {
              s_red[((wave * NT + nt) * 16 + g * 4 + j) * 2 + 0] = s;
              s_red[((wave * NT + nt) * 16 + g * 4 + j) * 2 + 1] = q;
            }
          }
        __syncthreads();
        if (tid < NT * 16) {
          const int nt = tid / 16, c = tid % 16;
          const int co = (cg * NT + nt) * 16 + c;
          if (co < a.Cout) {
            float s = 0.f, q = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
              s += s_red[((w * NT + nt) * 16 + c) * 2 + 0];
              q += s_red[((w * NT + nt) * 16 + c) * 2 + 1];
            }
            float* dst = a.stats_partial + ((size_t)tile_lin * a.Cout + co) * 2;
            dst[0] = s;
            dst[1] = q;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[r][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    tile_lin = ntile; chunk = nchunk; have = nhave;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// torch (Cout, Cin, KS, KS) fp32 -> [row group][sub-block][tap][nt][lane][4 floats]
__global__ void pack_conv2d_kernel(const float* __restrict__ w, float* __restrict__ out, int Cin, int Cin_pad, int Cout,
                                   int KS, int NT, int64_t total) {
  const int ntap = KS * KS, nsub = Cin_pad / 16;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i;
    const int j = r % 4; r /= 4;
    const int lane = r % 64; r /= 64;
    const int nt = r % NT; r /= NT;
    const int tap = r % ntap; r /= ntap;
    const int sub = r % nsub; r /= nsub;
    const int rgrp = (int)r;
    const int row = (rgrp * NT + nt) * 16 + (lane & 15);
    const int ci = sub * 16 + (lane >> 4) * 4 + j;
    float v = 0.f;
    if (row < Cout && ci < Cin) v = w[((size_t)row * Cin + ci) * ntap + tap];
    out[i] = v;
  }
}

int vx_pack_conv2d_mfma(const float* w_torch, float* w_packed, int Cin, int Cout, int KS, int64_t total, hipStream_t s) {
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pack_conv2d_kernel, dim3(blocks), dim3(256), 0, s, w_torch, w_packed, Cin, (int)conv2d_cin_padded(Cin), Cout, KS,
                     c2_config(KS, Cout).NT, total);
  VX_CHECK_LAUNCH("vx_pack_conv2d");
  return VX_OK;
}

template <int KS, int S, int NT, int NSUB, int TY>
static int launch_c2(const Conv2dRoute& r, const vx_conv2d_args& a, hipStream_t s) {
  static_assert(c2_geo(KS, S, NT, NSUB, TY).lds_bytes <= C2_LDS_BYTES, "LDS budget");
  Conv2dKArgs ka;
  ka.a = a;
  ka.OH = r.OH; ka.OW = r.OW; ka.tiles_x = r.tiles_x; ka.tiles_y = r.tiles_y; ka.nchunks = r.nchunks;
  ka.mx = r.mx; ka.my = r.my;
  const size_t lds = (size_t)r.lds_bytes;
  static size_t attr_lds = 0;
  auto kern = conv2d_mfma_kernel<KS, S, NT, NSUB, TY>;
  if (lds > attr_lds) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) VX_FAIL((int)e, "vx_conv2d: hipFuncSetAttribute(%zu B LDS): %s", lds, hipGetErrorString(e));
    attr_lds = lds;
  }
  static const char* kname = vx_conv2d_kname(r);
  vx_note_kernel(kname);
  hipLaunchKernelGGL(kern, dim3((unsigned)r.grid_x, (unsigned)r.grid_y), dim3(512), lds, s, ka);
  VX_CHECK_LAUNCH("vx_conv2d");
  return VX_OK;
}

// arguments validated and the instance chosen by conv2d_route
int vx_conv2d_mfma_launch(const Conv2dRoute& r, const vx_conv2d_args& a, hipStream_t s) {
  switch (conv2d_key_of(r.p)) {
#define C2_CASE(...) case conv2d_key(__VA_ARGS__): return launch_c2<__VA_ARGS__>(r, a, s);
    C2_INSTANCES(C2_CASE)
#undef C2_CASE
  }
  VX_FAIL(VX_E_SHAPE, "vx_conv2d: no such instance");
}
