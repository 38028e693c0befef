// K2 finalize + K2/K3/K4/K5/K7 apply.
//   vx_instnorm_finalize : per-(sample, channel) reduction of the conv epilogue's per-tile
//                          (sum, sumsq) partials in float64 -> mean, rstd (biased var, eps).
//   vx_norm_act_drop_pool: y = Dropout(LeakyReLU((x - mean) * rstd)); writes y with an arbitrary
//                          channel pitch/offset (the skip half of the decoder concat buffer) and the
//                          2x2x2 max-pool of y.  Pure streaming: 16-byte vectors, HBM-bound.
// Host side: every argument check, instance choice and launch geometry is in stream3d_route.h; an entry point is its route, then
// the kernel family's launcher with the descriptor.
#include "s16_common.h"
#include "stream3d_route.h"

// a route's refusal becomes the library's error
static int routed(int rc, const Stream3dRoute& r) {
  if (rc != VX_OK) vx_set_error("%s", r.err);
  return rc;
}
// the route's name, formatted once per launcher instance (a function-local static at each call) and kept for the process
static const char* s3_kname(const Stream3dRoute& r) {
  char buf[96];
  stream3d_route_name(r, buf, (int)sizeof(buf));
  return vx_kname("%s", buf);
}

__global__ __launch_bounds__(64) void instnorm_finalize_kernel(const float* __restrict__ partial, int ntiles, int C,
                                                               double inv_count, float eps, float* __restrict__ mean,
                                                               float* __restrict__ rstd) {
  const int n = blockIdx.x / C, c = blockIdx.x % C;
  const float* p = partial + ((size_t)n * ntiles * C + c) * 2;
  double s = 0.0, q = 0.0;
  for (int t = threadIdx.x; t < ntiles; t += 64) {
    s += (double)p[(size_t)t * C * 2 + 0];
    q += (double)p[(size_t)t * C * 2 + 1];
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    s += __shfl_xor(s, off, 64);
    q += __shfl_xor(q, off, 64);
  }
  if (threadIdx.x == 0) {
    const double mu = s * inv_count;
    double var = q * inv_count - mu * mu;
    if (var < 0.0) var = 0.0;
    mean[blockIdx.x] = (float)mu;
    rstd[blockIdx.x] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

extern "C" int vx_instnorm_finalize(const float* stats_partial, int N, int ntiles, int C, int64_t nvox, float eps,
                                    float* mean, float* rstd, vx_stream_t stream) {
  Stream3dRoute r;
  if (const int rc = routed(stream3d_finalize_route(stats_partial, N, ntiles, C, nvox, mean, rstd, &r), r)) return rc;
  static const char* kname = s3_kname(r);
  vx_note_kernel(kname);
  hipLaunchKernelGGL(instnorm_finalize_kernel, dim3((unsigned)r.grid_x), dim3(64), 0, (hipStream_t)stream,
                     stats_partial, ntiles, C, 1.0 / (double)nvox, eps, mean, rstd);
  VX_CHECK_LAUNCH("vx_instnorm_finalize");
  return VX_OK;
}

// Round 5: the statistics of ONE sample reduced by the consuming streaming pass itself (vx_stat_src): every workgroup of
// sample n sums the sample's partials (tiles x C x 2 floats, L2-resident) in float64 -- L = 256 / C threads per channel over
// strided tiles, then one thread per channel over the L partial sums -- and keeps mean / rstd in LDS; the workgroups with
// blockIdx.x == 0 also write them out for later readers.  Same formula as instnorm_finalize_kernel (biased variance, eps inside
// the root); the float64 summation ORDER differs, i.e. the float results agree to the last bit except on a rounding boundary.
// The four instnorm_finalize launches in front of these passes (first block's pre-split, vx_pool_finish_z, the two normalise +
// pool passes of the deep levels) are gone: 33 -> 29 launches per forward.
struct StatSrc { const float* partial; int tiles; double inv_count; float eps; float* mean_out; float* rstd_out; };
__device__ __forceinline__ void vx_block_instnorm(const StatSrc& st, int n, int C, bool write, float* s_mu, float* s_rs, double* s_part) {
  const float* p = st.partial + (size_t)n * st.tiles * C * 2;
  const int tid = threadIdx.x;
  for (int c0 = 0; c0 < C; c0 += 256) {
    const int cw = C - c0 < 256 ? C - c0 : 256;
    int L = 1;
    while (2 * L * cw <= 256) L *= 2;
    const int c = tid % cw, sub = tid / cw;
    double s = 0.0, q = 0.0;
    if (sub < L) {
      // (four tiles' loads in flight per trip: the trips are dependent L2 round trips)
      const size_t tstride = (size_t)L * C * 2;
      const float* e = p + ((size_t)sub * C + c0 + c) * 2;
      int t = sub;
      for (; t + 3 * L < st.tiles; t += 4 * L, e += 4 * tstride) {
        const f32x2 v0 = *reinterpret_cast<const f32x2*>(e), v1 = *reinterpret_cast<const f32x2*>(e + tstride);
        const f32x2 v2 = *reinterpret_cast<const f32x2*>(e + 2 * tstride), v3 = *reinterpret_cast<const f32x2*>(e + 3 * tstride);
        s += (double)v0[0]; q += (double)v0[1];
        s += (double)v1[0]; q += (double)v1[1];
        s += (double)v2[0]; q += (double)v2[1];
        s += (double)v3[0]; q += (double)v3[1];
      }
      for (; t < st.tiles; t += L, e += tstride) {
        const f32x2 v0 = *reinterpret_cast<const f32x2*>(e);
        s += (double)v0[0];
        q += (double)v0[1];
      }
    }
    s_part[tid] = s;
    s_part[256 + tid] = q;
    __syncthreads();
    if (tid < cw) {
      double S = 0.0, Q = 0.0;
      for (int k = 0; k < L; ++k) { S += s_part[k * cw + tid]; Q += s_part[256 + k * cw + tid]; }
      const double mu = S * st.inv_count;
      double var = Q * st.inv_count - mu * mu;
      if (var < 0.0) var = 0.0;
      const float m = (float)mu, r = (float)(1.0 / sqrt(var + (double)st.eps));
      s_mu[c0 + tid] = m;
      s_rs[c0 + tid] = r;
      if (write && st.mean_out) st.mean_out[(size_t)n * C + c0 + tid] = m;
      if (write && st.rstd_out) st.rstd_out[(size_t)n * C + c0 + tid] = r;
    }
    __syncthreads();
  }
}
// the device's form of a checked vx_stat_src (null: the pass takes mean / rstd tables)
static StatSrc stat_src(const vx_stat_src* st) {
  if (!st) return StatSrc{};
  return StatSrc{st->stats_partial, st->tiles, 1.0 / (double)st->count, st->eps, st->mean_out, st->rstd_out};
}

// One thread = one 16-byte piece (4 channels of one voxel) of a full-resolution ROW; consecutive lanes hold
// consecutive pieces, so every load/store instruction of a wave is one contiguous 1 KiB segment of the row.
// POOL: the thread handles the same piece of the 4 rows (2z+dz, 2y+dy) of a 2x2 row bundle, takes their max,
// exchanges with the lane that holds the x-neighbour voxel (C/4 lanes away: one cross-lane shuffle) and the
// even-x lanes store the pooled piece.  Input sample = n / x_repeat: the T MC-dropout samples of a volume share
// the first layer's conv output and statistics (same input, dropout comes after), so contr_1_1 is computed once
// per volume and only this kernel fans it out into T differently-dropped copies.
// Index decode: blockIdx.y = sample, the piece index within the sample is 32-bit and is split with exact
// multiply-high divisions (magic = 2^32 / d + 1, exact while index * d < 2^32 -- checked by the launcher); the
// original int64 % and / chain cost ~300 VALU instructions per piece and made the write-only fan-out kernel
// instruction-bound at 2.7 TB/s.
struct NormDecode { unsigned per_sample, mPW, mC4, mH; };   // magic 0 = divisor 1
// fp16 range word (vx_conv3d_args.range_flag): one atomic per wave, and only for magnitudes within a factor two of the limit
__device__ __forceinline__ void vx_range_report(uint32_t* flag, float rmax) {
  if (!flag) return;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) rmax = fmaxf(rmax, __shfl_xor(rmax, off, 64));
  if ((threadIdx.x & 63) == 0 && !(rmax < 32768.f)) atomicMax(flag, __float_as_uint(rmax));
}
// WIDE (pooling with more than 128 channels): the x-neighbour's piece would sit in another wave, so a thread takes
// BOTH voxels of an x-pair (a row then has W/2 * C/4 work items) and no shuffle is needed.
template <bool POOL, bool WIDE = false, bool FOLD = false>
__global__ __launch_bounds__(256) void norm_act_drop_pool_kernel(vx_norm_args a, int x_repeat, NormDecode dc, StatSrc st) {
  const int C4 = a.C / 4;
  const int PW = (WIDE ? a.W / 2 : a.W) * C4;  // work items per row
  const int n = blockIdx.y;
  const int RH = POOL ? a.H / 2 : a.H;   // rows (row bundles) per z
  alignas(16) __shared__ float s_mu[FOLD ? VX_STAT_MAXC : 4], s_rs[FOLD ? VX_STAT_MAXC : 4];   // (read as 16-byte vectors)
  __shared__ double s_part[FOLD ? 512 : 1];
  if constexpr (FOLD) vx_block_instnorm(st, n / x_repeat, a.C, blockIdx.x == 0, s_mu, s_rs, s_part);
  float rmax = 0.f;   // largest |value| stored: range guard of the split-fp16 consumers when nothing normalises (a.range_flag)
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < dc.per_sample; i += gridDim.x * 256u) {
    const unsigned row = vx_magic_div(i, dc.mPW);       // i / PW
    const int p = (int)(i - row * (unsigned)PW);
    const int xq = (int)vx_magic_div((unsigned)p, dc.mC4), c = (p - xq * C4) * 4;
    const int bz = (int)vx_magic_div(row, dc.mH);       // row / RH
    const int by = (int)(row - (unsigned)bz * (unsigned)RH);
    const int ns = n / x_repeat;
    f32x4 mu = (f32x4){0.f, 0.f, 0.f, 0.f}, rs = (f32x4){1.f, 1.f, 1.f, 1.f};
    if constexpr (FOLD) {
      mu = *reinterpret_cast<const f32x4*>(s_mu + c);
      rs = *reinterpret_cast<const f32x4*>(s_rs + c);
    } else if (a.mean) {
      mu = *reinterpret_cast<const f32x4*>(a.mean + (size_t)ns * a.C + c);
      rs = *reinterpret_cast<const f32x4*>(a.rstd + (size_t)ns * a.C + c);
    }
    const vx_dkey dkey = vx_drop_key(vx_seed_of(a, a.drop_seed), a.drop_layer, (uint32_t)n);
    f32x4 mx = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    constexpr int NR = POOL ? (WIDE ? 8 : 4) : 1;
    f32x4 v[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const int z = POOL ? bz * 2 + ((k >> 1) & 1) : bz;
      const int y = POOL ? by * 2 + (k & 1) : by;
      const int x = WIDE ? 2 * xq + (k >> 2) : xq;
      if (a.x_xblk) {   // the raw tensor sits in a concat buffer's half (dense blocks of xb voxels)
        const size_t srow = (size_t)(ns * a.D + z) * a.H + y;
        const int xb = a.x_xblk;
        v[k] = *reinterpret_cast<const f32x4*>(a.x + srow * (2 * (size_t)a.W * a.C) + ((x / xb) * 2 + a.x_half) * xb * a.C +
                                               (x % xb) * a.C + c);
      } else {
        const size_t svox = ((size_t)(ns * a.D + z) * a.H + y) * a.W + x;
        v[k] = *reinterpret_cast<const f32x4*>(a.x + svox * a.x_pitch + c);
      }
    }
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const int z = POOL ? bz * 2 + ((k >> 1) & 1) : bz;
      const int y = POOL ? by * 2 + (k & 1) : by;
      const int x = WIDE ? 2 * xq + (k >> 2) : xq;
      const size_t vox = ((size_t)(n * a.D + z) * a.H + y) * a.W + x;
      f32x4 t = (v[k] - mu) * rs;
      if (a.act == VX_ACT_LRELU) {
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = fmaxf(t[j], 0.01f * t[j]);
      } else if (a.act == VX_ACT_RELU) {
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = fmaxf(t[j], 0.f);
      }
      if (a.drop_mode == VX_DROP_HASH) {
        const uint32_t e = (uint32_t)(((z * a.H + y) * a.W + x) * a.C + c);
        const uint32_t bits = vx_drop_bits4(dkey, e);
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] *= __uint_as_float((bits << (30 - j)) & 0x40000000u);  // keep ? 2.0f : 0.0f
      } else if (a.drop_mode == VX_DROP_MASK) {
        const uint32_t mk = *reinterpret_cast<const uint32_t*>(a.drop_mask + vox * a.C + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = ((mk >> (8 * j)) & 0xFFu) ? 2.f * t[j] : 0.f;
      }
      if (a.range_flag) rmax = fmaxf(fmaxf(rmax, fmaxf(fabsf(t[0]), fabsf(t[1]))), fmaxf(fabsf(t[2]), fabsf(t[3])));
      if (!a.out) {
        // pooled tensor only
      } else if (a.out_xblk) {
        // concat buffer [N][D][H][W/xb][2][xb][C]: this kernel's half as dense blocks of xb voxels
        const size_t row = (size_t)(n * a.D + z) * a.H + y;
        const int xb = a.out_xblk;
        *reinterpret_cast<f32x4*>(a.out + row * (2 * (size_t)a.W * a.C) + ((x / xb) * 2 + a.out_half) * xb * a.C +
                                  (x % xb) * a.C + c) = t;
      } else {
        *reinterpret_cast<f32x4*>(a.out + vox * a.out_pitch + a.out_coff + c) = t;
      }
      if (POOL) {
#pragma unroll
        for (int j = 0; j < 4; ++j) mx[j] = fmaxf(mx[j], t[j]);
      }
    }
    if (POOL && WIDE) {
      const size_t pv = ((size_t)(n * (a.D / 2) + bz) * (a.H / 2) + by) * (a.W / 2) + xq;
      *reinterpret_cast<f32x4*>(a.pool_out + pv * a.pool_pitch + c) = mx;
    } else if (POOL) {
      const int x = xq;
      // x-neighbour voxel's piece with the same channels sits C4 pieces (= lanes) away
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = __shfl_xor(mx[j], C4, 64);
      if ((x & 1) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) mx[j] = fmaxf(mx[j], o[j]);
        const size_t pv = ((size_t)(n * (a.D / 2) + bz) * (a.H / 2) + by) * (a.W / 2) + (x >> 1);
        *reinterpret_cast<f32x4*>(a.pool_out + pv * a.pool_pitch + c) = mx;
      }
    }
  }
  vx_range_report(a.range_flag, rmax);
}

// Fan-out variant (MC-dropout first layer: x_repeat = T samples share one source volume, no pooling): one thread
// per SOURCE piece -- one load and one normalise + activation, then T dropout patterns and T fire-and-forget
// stores.  The per-sample kernel above re-read and re-normalised the source T times with one 16-byte load in
// flight per thread: latency-bound at 3.2 TB/s written; this one streams at the write roof.
__global__ __launch_bounds__(256) void norm_act_drop_fanout_kernel(vx_norm_args a, int x_repeat, NormDecode dc) {
  const int C4 = a.C / 4;
  const int PW = a.W * C4;
  const int ns = blockIdx.y;
  const size_t out_sample = (size_t)a.D * a.H * a.W * (a.out_xblk ? 2 * a.C : a.out_pitch);
  const int xs = a.out_xblk ? __builtin_ctz((unsigned)a.out_xblk) : 0;
  float rmax = 0.f;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < dc.per_sample; i += gridDim.x * 256u) {
    const unsigned row = vx_magic_div(i, dc.mPW);
    const int p = (int)(i - row * (unsigned)PW);
    const int x = (int)vx_magic_div((unsigned)p, dc.mC4), c = (p - x * C4) * 4;
    const int z = (int)vx_magic_div(row, dc.mH);
    const int y = (int)(row - (unsigned)z * (unsigned)a.H);
    f32x4 mu = (f32x4){0.f, 0.f, 0.f, 0.f}, rs = (f32x4){1.f, 1.f, 1.f, 1.f};
    if (a.mean) {
      mu = *reinterpret_cast<const f32x4*>(a.mean + (size_t)ns * a.C + c);
      rs = *reinterpret_cast<const f32x4*>(a.rstd + (size_t)ns * a.C + c);
    }
    const size_t svox = ((size_t)(ns * a.D + z) * a.H + y) * a.W + x;
    f32x4 t0 = (*reinterpret_cast<const f32x4*>(a.x + svox * a.x_pitch + c) - mu) * rs;
    if (a.act == VX_ACT_LRELU) {
#pragma unroll
      for (int j = 0; j < 4; ++j) t0[j] = fmaxf(t0[j], 0.01f * t0[j]);
    } else if (a.act == VX_ACT_RELU) {
#pragma unroll
      for (int j = 0; j < 4; ++j) t0[j] = fmaxf(t0[j], 0.f);
    }
    // (the dropout's factor 2 included: what the T samples store is at most twice this)
    if (a.range_flag) rmax = fmaxf(fmaxf(rmax, 2.f * fmaxf(fabsf(t0[0]), fabsf(t0[1]))), 2.f * fmaxf(fabsf(t0[2]), fabsf(t0[3])));
    const uint32_t e = (uint32_t)(((z * a.H + y) * a.W + x) * a.C + c);
    size_t off;   // float offset of the piece within a sample's output
    if (a.out_xblk)
      off = ((size_t)z * a.H + y) * (2 * (size_t)a.W * a.C) + ((((x >> xs) * 2 + a.out_half) << xs) + (x & (a.out_xblk - 1))) * a.C + c;
    else
      off = (((size_t)z * a.H + y) * a.W + x) * a.out_pitch + a.out_coff + c;
    for (int k = 0; k < x_repeat; ++k) {
      const int n = ns * x_repeat + k;
      f32x4 t = t0;
      if (a.drop_mode == VX_DROP_HASH) {
        const uint32_t bits = vx_drop_bits4(vx_drop_key(vx_seed_of(a, a.drop_seed), a.drop_layer, (uint32_t)n), e);
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] *= __uint_as_float((bits << (30 - j)) & 0x40000000u);
      } else if (a.drop_mode == VX_DROP_MASK) {
        const uint32_t mk = *reinterpret_cast<const uint32_t*>(a.drop_mask + (size_t)n * a.D * a.H * a.W * a.C + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = ((mk >> (8 * j)) & 0xFFu) ? 2.f * t[j] : 0.f;
      }
      *reinterpret_cast<f32x4*>(a.out + (size_t)n * out_sample + off) = t;
    }
  }
  vx_range_report(a.range_flag, rmax);
}

template <bool POOL, bool WIDE, bool FOLD>
static void launch_norm_instance(const Stream3dRoute& r, const vx_norm_args& a, int x_repeat, const NormDecode& dc, const StatSrc& st, hipStream_t s) {
  static const char* kname = s3_kname(r);
  vx_note_kernel(kname);
  hipLaunchKernelGGL((norm_act_drop_pool_kernel<POOL, WIDE, FOLD>), dim3(r.grid_x, r.grid_y), dim3(256), 0, s, a, x_repeat, dc, st);
}

static int norm_route_or_fail(const vx_norm_args* ap, int x_repeat, const vx_stat_src* stsrc, Stream3dRoute* r) {
  if (!ap) VX_FAIL(VX_E_NULL, "vx_norm_act_drop_pool: null args");
  return routed(stream3d_norm_route(*ap, x_repeat, stsrc, r), *r);
}

// the three forms of the pass: one route, one launcher
static int launch_norm(const vx_norm_args* ap, int x_repeat, const vx_stat_src* stsrc, vx_stream_t stream) {
  Stream3dRoute r;
  if (const int rc = norm_route_or_fail(ap, x_repeat, stsrc, &r)) return rc;
  const vx_norm_args& a = *ap;
  hipStream_t s = (hipStream_t)stream;
  const NormDecode dc = {r.pieces, r.mPW, r.mC4, r.mH};
  const StatSrc st = stat_src(stsrc);
  if (r.kernel == S3_FANOUT) {
    static const char* kname = s3_kname(r);
    vx_note_kernel(kname);
    hipLaunchKernelGGL(norm_act_drop_fanout_kernel, dim3(r.grid_x, r.grid_y), dim3(256), 0, s, a, x_repeat, dc);
  } else {
#define NORM_LAUNCH_CASE(P, W, F) case stream3d_key(P, W, F): launch_norm_instance<P != 0, W != 0, F != 0>(r, a, x_repeat, dc, st, s); break;
    switch (stream3d_key(r.pool, r.wide, r.fold)) { STREAM3D_NORM_INSTANCES(NORM_LAUNCH_CASE) }
#undef NORM_LAUNCH_CASE
  }
  VX_CHECK_LAUNCH("vx_norm_act_drop_pool");
  return VX_OK;
}

extern "C" int vx_norm_act_drop_pool(const vx_norm_args* ap, vx_stream_t stream) { return launch_norm(ap, 1, nullptr, stream); }
extern "C" int vx_norm_act_drop_pool_bcast(const vx_norm_args* ap, int x_repeat, vx_stream_t stream) {
  return launch_norm(ap, x_repeat, nullptr, stream);
}
extern "C" int vx_norm_act_drop_pool_stats(const vx_norm_args* ap, const vx_stat_src* st, vx_stream_t stream) {
  if (!st) VX_FAIL(VX_E_NULL, "vx_norm_act_drop_pool_stats: null statistics source");
  return launch_norm(ap, 1, st, stream);
}
extern "C" int vx_norm_act_drop_pool_route(const vx_norm_args* ap, int x_repeat, const vx_stat_src* st, char* kernel_name, int cap,
                                           vx_norm_route_info* info) {
  Stream3dRoute r;
  if (const int rc = norm_route_or_fail(ap, x_repeat, st, &r)) return rc;
  if (kernel_name && cap > 0) stream3d_route_name(r, kernel_name, cap);
  if (info) *info = {r.grid_x, r.grid_y, r.pieces, r.mPW, r.mC4, r.mH};
  return VX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// The keep-bits VX_DROP_HASH uses, written out as a VX_DROP_MASK-style mask: mask[n][e] = bit of element e of sample n
// of dropout layer `layer` under `seed` (e = channels-last linear index, voxel * C + c -- what every kernel hashes).
// Lets a caller replay a hash-dropout run with explicit masks (parity tests feed them to the float64 oracle).
__global__ __launch_bounds__(256) void drop_hash_mask_kernel(uint32_t seed, uint32_t layer, int N, int64_t per,
                                                             uint8_t* __restrict__ out) {
  const int64_t groups = per / 4;
  const int64_t total = (int64_t)N * groups;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / groups, g = i - n * groups;
    const uint32_t bits = vx_drop_bits4(vx_drop_key(seed, layer, (uint32_t)n), (uint32_t)(4 * g));
    const uint32_t v = (bits & 1u) | ((bits >> 1 & 1u) << 8) | ((bits >> 2 & 1u) << 16) | ((bits >> 3 & 1u) << 24);
    *reinterpret_cast<uint32_t*>(out + n * per + 4 * g) = v;
  }
}

extern "C" int vx_drop_hash_mask(uint32_t seed, uint32_t layer, int N, int64_t elems_per_sample, uint8_t* mask,
                                 vx_stream_t stream) {
  Stream3dRoute r;
  if (const int rc = routed(stream3d_hash_mask_route(N, elems_per_sample, mask, &r), r)) return rc;
  hipLaunchKernelGGL(drop_hash_mask_kernel, dim3(r.grid_x), dim3(256), 0, (hipStream_t)stream, seed, layer, N, elems_per_sample, mask);
  VX_CHECK_LAUNCH("vx_drop_hash_mask");
  return VX_OK;
}

// The second half of a pooled contract block whose conv left window maxima and any-dropped bits (vx_conv3d_args.pool_out):
// one thread = one 16-byte piece (4 channels of one pooled voxel, C = 8).
__global__ __launch_bounds__(256) void pool_finish_kernel(const float* __restrict__ raw, const uint32_t* __restrict__ flags,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          float* __restrict__ out, int out_pitch, unsigned pieces, float s) {
  const int n = blockIdx.y;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < pieces; i += gridDim.x * 256u) {
    const unsigned vox = i >> 1, q = i & 1u;
    const size_t pv = (size_t)n * (pieces >> 1) + vox;
    const f32x4 m = *reinterpret_cast<const f32x4*>(raw + pv * 8 + q * 4);
    const uint32_t fl = flags[pv * 2 + q];
    const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + (size_t)n * 8 + q * 4);
    const f32x4 rs = *reinterpret_cast<const f32x4*>(rstd + (size_t)n * 8 + q * 4);
    f32x4 t = (m - mu) * rs;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = fmaxf(t[j], 0.01f * t[j]) * s;       // as vx_norm_act_drop_pool: normalise, LeakyReLU, then the dropout's 2
      if ((fl >> j) & 1u) v = fmaxf(v, 0.f);          // a dropped element contributes 0 to the window
      t[j] = v;
    }
    *reinterpret_cast<f32x4*>(out + pv * out_pitch + q * 4) = t;
  }
}

// vx_pool_finish_z: the 16-channel z-column kernel leaves the (y, x) half of every window per z-plane (values_amd.h); one
// thread = one 16-byte piece of a pooled voxel: maximum / OR over the z pair, then pool_finish_kernel's arithmetic
template <bool FOLD>
__global__ __launch_bounds__(256) void pool_finish_z_kernel(const float* __restrict__ raw, const uint32_t* __restrict__ flags,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            float* __restrict__ out, int out_pitch, unsigned Dp, unsigned pv_plane, float s,
                                                            StatSrc st) {
  const int n = blockIdx.y;
  alignas(16) __shared__ float s_mu[FOLD ? 16 : 4], s_rs[FOLD ? 16 : 4];      // (read as 16-byte vectors)
  __shared__ double s_part[FOLD ? 512 : 1];
  if constexpr (FOLD) vx_block_instnorm(st, n, 16, blockIdx.x == 0, s_mu, s_rs, s_part);
  // this sample's 16 means / reciprocal deviations: the workgroup's own reduction (LDS) or row n of the caller's tables
  const float* mu_n = FOLD ? s_mu : mean + (size_t)n * 16;
  const float* rs_n = FOLD ? s_rs : rstd + (size_t)n * 16;
  const unsigned pieces = Dp * pv_plane * 4u;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < pieces; i += gridDim.x * 256u) {
    const unsigned vox = i >> 2, q = i & 3u;
    const unsigned zp = vox / pv_plane, r = vox - zp * pv_plane;
    const size_t v0 = ((size_t)n * 2 * Dp + 2 * zp) * pv_plane + r, v1 = v0 + pv_plane;
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(raw + v0 * 16 + q * 4);
    const f32x4 a1 = *reinterpret_cast<const f32x4*>(raw + v1 * 16 + q * 4);
    const uint32_t fl = flags[v0 * 4 + q] | flags[v1 * 4 + q];
    const f32x4 mu = *reinterpret_cast<const f32x4*>(mu_n + q * 4);
    const f32x4 rs = *reinterpret_cast<const f32x4*>(rs_n + q * 4);
    f32x4 t;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float tt = (fmaxf(a0[j], a1[j]) - mu[j]) * rs[j];
      float v = fmaxf(tt, 0.01f * tt) * s;
      if ((fl >> j) & 1u) v = fmaxf(v, 0.f);
      t[j] = v;
    }
    *reinterpret_cast<f32x4*>(out + ((size_t)n * Dp * pv_plane + vox) * out_pitch + q * 4) = t;
  }
}

// vx_prenorm_split: one thread = one 16-byte piece, in place (values_amd.h)
template <bool FOLD>
__global__ __launch_bounds__(256) void prenorm_split_kernel(float* __restrict__ x, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, unsigned pieces, float scale, StatSrc st) {
  const int n = blockIdx.y;
  alignas(16) __shared__ float s_mu[FOLD ? 8 : 4], s_rs[FOLD ? 8 : 4];
  __shared__ double s_part[FOLD ? 512 : 1];
  if constexpr (FOLD) vx_block_instnorm(st, n, 8, blockIdx.x == 0, s_mu, s_rs, s_part);
  const float* mu_n = FOLD ? s_mu : mean + (size_t)n * 8;
  const float* rs_n = FOLD ? s_rs : rstd + (size_t)n * 8;
  f32x4* xs = reinterpret_cast<f32x4*>(x) + (size_t)n * pieces;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < pieces; i += gridDim.x * 256u) {
    const int c = (i & 1u) * 4;
    const f32x4 mu = *reinterpret_cast<const f32x4*>(mu_n + c);
    f32x4 sc = *reinterpret_cast<const f32x4*>(rs_n + c);
    f32x4 v = xs[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float t = (v[j] - mu[j]) * (sc[j] * scale);     // the z-column kernel's prologue arithmetic, bit for bit
      v[j] = fmaxf(t, 0.01f * t);
    }
    f16x4 hi, lo;
    vx_split4(v, hi, lo);
    f32x4 o;
    o[0] = __builtin_bit_cast(float, (f16x2){hi[0], hi[1]});
    o[1] = __builtin_bit_cast(float, (f16x2){hi[2], hi[3]});
    o[2] = __builtin_bit_cast(float, (f16x2){lo[0], lo[1]});
    o[3] = __builtin_bit_cast(float, (f16x2){lo[2], lo[3]});
    xs[i] = o;
  }
}

// ---- the small passes: the plain and the _stats form of a pass are one route and one launcher, FOLD the kernel's own switch ----
template <bool FOLD>
static int launch_split(const char* who, float* x, const float* mean, const float* rstd, const vx_stat_src* stsrc, int N, int64_t nvox,
                        float scale, vx_stream_t stream) {
  Stream3dRoute r;
  if (const int rc = routed(stream3d_split_route(who, x, mean, rstd, FOLD, stsrc, N, nvox, &r), r)) return rc;
  static const char* kname = s3_kname(r);
  vx_note_kernel(kname);
  hipLaunchKernelGGL(prenorm_split_kernel<FOLD>, dim3(r.grid_x, r.grid_y), dim3(256), 0, (hipStream_t)stream, x, mean, rstd, r.pieces, scale,
                     stat_src(stsrc));
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}
extern "C" int vx_prenorm_split(float* x, const float* mean, const float* rstd, int N, int64_t nvox, float scale, vx_stream_t stream) {
  return launch_split<false>("vx_prenorm_split", x, mean, rstd, nullptr, N, nvox, scale, stream);
}
extern "C" int vx_prenorm_split_stats(float* x, const vx_stat_src* stsrc, int N, int64_t nvox, float scale, vx_stream_t stream) {
  return launch_split<true>("vx_prenorm_split_stats", x, nullptr, nullptr, stsrc, N, nvox, scale, stream);
}

extern "C" int vx_pool_finish(const float* pool_raw, const uint32_t* pool_flags, const float* mean, const float* rstd,
                              float* out, int out_pitch, int N, int64_t voxels_per_sample, int drop_scale2,
                              vx_stream_t stream) {
  Stream3dRoute r;
  if (const int rc = routed(stream3d_finish_route(pool_raw, pool_flags, mean, rstd, out, out_pitch, N, voxels_per_sample, &r), r)) return rc;
  static const char* kname = s3_kname(r);
  vx_note_kernel(kname);
  hipLaunchKernelGGL(pool_finish_kernel, dim3(r.grid_x, r.grid_y), dim3(256), 0, (hipStream_t)stream, pool_raw, pool_flags, mean,
                     rstd, out, out_pitch, r.pieces, drop_scale2 ? 2.f : 1.f);
  VX_CHECK_LAUNCH("vx_pool_finish");
  return VX_OK;
}

template <bool FOLD>
static int launch_finish_z(const char* who, const float* pool_raw, const uint32_t* pool_flags, const float* mean, const float* rstd,
                           const vx_stat_src* stsrc, float* out, int out_pitch, int N, int Dp, int64_t plane_voxels, int drop_scale2,
                           vx_stream_t stream) {
  Stream3dRoute r;
  if (const int rc = routed(stream3d_finish_z_route(who, pool_raw, pool_flags, mean, rstd, FOLD, stsrc, out, out_pitch, N, Dp, plane_voxels, &r), r))
    return rc;
  static const char* kname = s3_kname(r);
  vx_note_kernel(kname);
  hipLaunchKernelGGL(pool_finish_z_kernel<FOLD>, dim3(r.grid_x, r.grid_y), dim3(256), 0, (hipStream_t)stream, pool_raw, pool_flags, mean,
                     rstd, out, out_pitch, (unsigned)Dp, (unsigned)plane_voxels, drop_scale2 ? 2.f : 1.f, stat_src(stsrc));
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}
extern "C" int vx_pool_finish_z(const float* pool_raw, const uint32_t* pool_flags, const float* mean, const float* rstd,
                                float* out, int out_pitch, int N, int Dp, int64_t plane_voxels, int drop_scale2,
                                vx_stream_t stream) {
  return launch_finish_z<false>("vx_pool_finish_z", pool_raw, pool_flags, mean, rstd, nullptr, out, out_pitch, N, Dp, plane_voxels, drop_scale2, stream);
}
extern "C" int vx_pool_finish_z_stats(const float* pool_raw, const uint32_t* pool_flags, const vx_stat_src* stsrc, float* out,
                                      int out_pitch, int N, int Dp, int64_t plane_voxels, int drop_scale2, vx_stream_t stream) {
  return launch_finish_z<true>("vx_pool_finish_z_stats", pool_raw, pool_flags, nullptr, nullptr, stsrc, out, out_pitch, N, Dp, plane_voxels, drop_scale2,
                               stream);
}

extern "C" int vx_zero(void* p, int64_t bytes, vx_stream_t stream) {
  if (bytes < 0 || (!p && bytes > 0)) VX_FAIL(VX_E_NULL, "vx_zero: null pointer / negative size");
  if (bytes == 0) return VX_OK;
  const hipError_t e = hipMemsetAsync(p, 0, (size_t)bytes, (hipStream_t)stream);
  if (e != hipSuccess) VX_FAIL((int)e, "vx_zero: hipMemsetAsync(%lld B): %s", (long long)bytes, hipGetErrorString(e));
  return VX_OK;
}
