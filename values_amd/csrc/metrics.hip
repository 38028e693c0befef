// Segmentation-metric reductions that follow the maps in run_test (test_3D.py:250-358, 537-575):
//   * vx_mask_agreement : for a set of M label masks (the T per-sample argmax masks and the R rater masks of one
//     image), the class-wise agreement counts  I[i][j][c] = #{v : mask_i(v) == c and mask_j(v) == c}  of every pair.
//     Every hard Dice the reference asks torchmetrics for -- Dice(pred_t, gt_r), the pooled pred/gt, pred/pred and
//     gt/gt distances of the generalised energy distance, the per-rater and per-prediction maxima -- is a ratio of
//     sums of these integers (tp = I, fp = I[i][i] - I, fn = I[j][j] - I), so ONE pass over the masks replaces the
//     T*R + T*T + R*R + 2*T*R mask comparisons of calculate_ged.
//   * vx_soft_metric_sums : per rater and class  sum_v p_c [gt == c],  sum_v [gt == c],  sum_v p_c  and
//     sum_v log p_gt(v)  for SoftDiceLoss + NLLLoss of calculate_test_metrics (loss_modules.py:7-97).
// Both are HBM-bound scans of a few MB; integer counts are exact and order-independent, the float sums are
// accumulated in fp64 per workgroup and combined in a fixed order (deterministic).
#include "common.h"

constexpr int MA_MAXM = 32;   // masks per call
constexpr int MA_MAXC = 8;    // classes

__global__ __launch_bounds__(256) void mask_agreement_kernel(const uint8_t* __restrict__ masks, int M, int C, int64_t nvox,
                                                             unsigned long long* __restrict__ out) {
  __shared__ unsigned long long bm[4][MA_MAXC][MA_MAXM];   // per wave: lanes whose mask i has class c
  __shared__ unsigned cnt[MA_MAXM * MA_MAXM * MA_MAXC];     // workgroup counters [i][j][c]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int npair = M * M * C;
  for (int i = tid; i < npair; i += 256) cnt[i] = 0;
  __syncthreads();
  const int64_t nchunk = (nvox + 63) / 64;
  for (int64_t ch = (int64_t)blockIdx.x * 4 + wave; ch < nchunk; ch += (int64_t)gridDim.x * 4) {
    const int64_t v = ch * 64 + lane;
    for (int i = 0; i < M; ++i) {
      const int l = v < nvox ? (int)masks[(size_t)i * nvox + v] : -1;
      for (int c = 0; c < C; ++c) {
        const unsigned long long b = __ballot(l == c);
        if (lane == 0) bm[wave][c][i] = b;
      }
    }
    // (same wave: LDS operations complete in order, no barrier needed)
    for (int p = lane; p < M * M; p += 64) {
      const int i = p / M, j = p - i * M;
      for (int c = 0; c < C; ++c) {
        const unsigned n = (unsigned)__popcll(bm[wave][c][i] & bm[wave][c][j]);
        if (n) atomicAdd(&cnt[p * C + c], n);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < npair; i += 256)
    if (cnt[i]) atomicAdd(&out[i], (unsigned long long)cnt[i]);
}

extern "C" int vx_mask_agreement(const uint8_t* masks, int M, int C, int64_t nvox, uint64_t* counts, vx_stream_t stream) {
  if (M <= 0 || M > MA_MAXM || C <= 0 || C > MA_MAXC || nvox < 0)
    VX_FAIL(VX_E_SHAPE, "vx_mask_agreement: M=%d (1..%d) C=%d (1..%d)", M, MA_MAXM, C, MA_MAXC);
  if (!counts) VX_FAIL(VX_E_NULL, "vx_mask_agreement: null output");
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)M * M * C * sizeof(uint64_t), s);
  if (e != hipSuccess) VX_FAIL((int)e, "vx_mask_agreement: memset: %s", hipGetErrorString(e));
  if (nvox == 0) return VX_OK;
  if (!masks) VX_FAIL(VX_E_NULL, "vx_mask_agreement: null masks");
  const int64_t nchunk = (nvox + 63) / 64;
  int bx = (int)((nchunk + 3) / 4);
  if (bx > 1024) bx = 1024;
  // (32-bit workgroup counters: a workgroup would need 2^26 chunks = 4 G voxels of its own to wrap one)
  hipLaunchKernelGGL(mask_agreement_kernel, dim3(bx), dim3(256), 0, s, masks, M, C, nvox,
                     reinterpret_cast<unsigned long long*>(counts));
  VX_CHECK_LAUNCH("vx_mask_agreement");
  return VX_OK;
}

// ---- vx_mask_agreement_batched: the same counts for the B images of a 2D inference step and up to 32 classes -------------------
// (process_output of test_2D.py:205-244: Cityscapes / GTA, 19 classes + the appended "ignore" class, M = 1 + T + R masks per image)
// A 64-pixel run of a label mask holds a handful of classes, so a wave
//   1. takes the ballot of a mask only for the classes PRESENT in its 64 pixels (a scalar loop: the class of the first lane not yet
//      covered, one ballot, those lanes struck off) and leaves them in LDS with the mask's presence word;
//   2. gives every pair i <= j of masks to a lane, which walks the classes present in BOTH masks: popcount of the two ballots'
//      intersection, one LDS add into the workgroup's triangle of counters cnt[class][pair] (lanes of one class: consecutive banks).
// The workgroup adds its triangle to the image's full [M][M][C] array at the end, (i, j) and (j, i) from the same counter.
// LDS is static and below 64 KB for every (M, C): masks <= 16 take all 32 classes at once (MT = 16, CS = 32: 34 KB), more masks take
// the classes in two slices of 16 (MT = 32, CS = 16: 51 KB; blockIdx.y; a slice sees the other slice's labels as "no class").
// 32-bit workgroup counters: a counter grows by at most 64 per chunk, so a workgroup would need 2^26 chunks = 2^32 pixels of its own
// to wrap one; the launcher refuses nvox > 2^39 and gives an image of more than 2^16 chunks at least 256 workgroups, so a workgroup
// sees at most max(2^16, 2^33 / 256) = 2^25 chunks and no counter passes 2^31.
constexpr int MAB_MAXC = 32;
constexpr int64_t MAB_MAXVOX = (int64_t)1 << 39;

template <int MT, int CS>
__global__ __launch_bounds__(256) void mask_agreement_batched_kernel(const uint8_t* __restrict__ masks, int M, int C, int64_t nvox,
                                                                     int remap_from, int bx, unsigned long long* __restrict__ out) {
  constexpr int TRI = MT * (MT + 1) / 2;
  __shared__ unsigned long long bm[4][CS][MT];   // per wave: lanes whose mask i has class c0 + c (valid where pm[i] has bit c)
  __shared__ unsigned pm[4][MT];                 // per wave: classes of the slice present in mask i's 64 pixels
  __shared__ unsigned cnt[CS * TRI];             // workgroup counters [c][pair]
  __shared__ unsigned short pij[TRI];            // pair -> i | j << 8
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / bx, blk = blockIdx.x - b * bx;
  const int c0 = blockIdx.y * CS, cs = min(C - c0, CS);   // this workgroup's classes [c0, c0 + cs)
  const int tri = M * (M + 1) / 2;
  for (int p = tid; p < tri; p += 256) {
    int i = 0, r = p;
    while (r >= M - i) { r -= M - i; ++i; }
    pij[p] = (unsigned short)(i | ((i + r) << 8));
  }
  for (int k = tid; k < cs * tri; k += 256) cnt[k] = 0;
  __syncthreads();
  const uint8_t* img = masks + (size_t)b * M * nvox;
  const int64_t nchunk = (nvox + 63) / 64;
  for (int64_t ch = (int64_t)blk * 4 + wave; ch < nchunk; ch += (int64_t)bx * 4) {
    const int64_t v = ch * 64 + lane;
    for (int i0 = 0; i0 < M; i0 += 8) {
      int lab[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) lab[k] = (i0 + k < M && v < nvox) ? (int)img[(size_t)(i0 + k) * nvox + v] : 256;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (i0 + k >= M) break;
        const int l = (lab[k] == remap_from ? C - 1 : lab[k]) - c0;   // 256 = past the end: no class, never remapped
        unsigned long long rem = __ballot((unsigned)l < (unsigned)cs);
        unsigned present = 0;
        while (rem) {
          const int c = __builtin_amdgcn_readlane(l, __ffsll((long long)rem) - 1);
          const unsigned long long bal = __ballot(l == c);
          if (lane == 0) bm[wave][c][i0 + k] = bal;
          present |= 1u << c;
          rem &= ~bal;
        }
        if (lane == 0) pm[wave][i0 + k] = present;
      }
    }
    // (same wave: LDS operations complete in order; the fence only keeps the compiler from moving them across)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (int p = lane; p < tri; p += 64) {
      const int i = pij[p] & 255, j = pij[p] >> 8;
      unsigned both = pm[wave][i] & pm[wave][j];
      while (both) {
        const int c = __ffs((int)both) - 1;
        both &= both - 1;
        const unsigned n = (unsigned)__popcll(bm[wave][c][i] & bm[wave][c][j]);
        if (n) atomicAdd(&cnt[c * tri + p], n);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  __syncthreads();
  unsigned long long* o = out + (size_t)b * M * M * C;
  for (int k = tid; k < cs * tri; k += 256) {
    const unsigned n = cnt[k];
    if (!n) continue;
    const int c = k / tri, p = k - c * tri;
    const int i = pij[p] & 255, j = pij[p] >> 8;
    atomicAdd(&o[((size_t)i * M + j) * C + c0 + c], (unsigned long long)n);
    if (i != j) atomicAdd(&o[((size_t)j * M + i) * C + c0 + c], (unsigned long long)n);
  }
}

extern "C" int vx_mask_agreement_batched(const uint8_t* masks, int B, int M, int C, int64_t nvox, int remap_from, uint64_t* counts,
                                         vx_stream_t stream) {
  if (B <= 0 || M <= 0 || M > MA_MAXM || C <= 0 || C > MAB_MAXC || nvox < 0 || nvox > MAB_MAXVOX)
    VX_FAIL(VX_E_SHAPE, "vx_mask_agreement_batched: B=%d (>= 1) M=%d (1..%d) C=%d (1..%d) nvox=%lld (0..2^39)", B, M, MA_MAXM, C,
            MAB_MAXC, (long long)nvox);
  if (!counts) VX_FAIL(VX_E_NULL, "vx_mask_agreement_batched: null output");
  if (remap_from < 0 || remap_from > 255) remap_from = -1;   // no uint8 label: nothing is remapped
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)B * M * M * C * sizeof(uint64_t), s);
  if (e != hipSuccess) VX_FAIL((int)e, "vx_mask_agreement_batched: memset: %s", hipGetErrorString(e));
  if (nvox == 0) return VX_OK;
  if (!masks) VX_FAIL(VX_E_NULL, "vx_mask_agreement_batched: null masks");
  const bool wide = M > 16;                              // more than 16 masks: 16 classes per workgroup, two slices above 16 classes
  const int slices = wide ? (C + 15) / 16 : 1;
  // workgroups per image: four chunks per wave before the flush where the image has them, about 2048 workgroups per launch,
  // never fewer than 256 for an image of more than 2^16 chunks (the counter bound above)
  const int64_t nchunk = (nvox + 63) / 64;
  int64_t bx = (nchunk + 15) / 16;
  const int64_t share = 2048 / ((int64_t)B * slices);
  if (bx > share) bx = share;
  if (nchunk > 65536 && bx < 256) bx = 256;
  if (bx < 1) bx = 1;
  if ((int64_t)B * bx > 0x7fffffff) VX_FAIL(VX_E_SHAPE, "vx_mask_agreement_batched: B=%d images of %lld pixels", B, (long long)nvox);
  const dim3 grid((unsigned)(B * bx), (unsigned)slices);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
  if (wide)
    hipLaunchKernelGGL((mask_agreement_batched_kernel<32, 16>), grid, dim3(256), 0, s, masks, M, C, nvox, remap_from, (int)bx, out);
  else
    hipLaunchKernelGGL((mask_agreement_batched_kernel<16, 32>), grid, dim3(256), 0, s, masks, M, C, nvox, remap_from, (int)bx, out);
  VX_CHECK_LAUNCH("vx_mask_agreement_batched");
  return VX_OK;
}

// out[r][c][0] = sum p_c [gt_r == c], [1] = sum [gt_r == c], [2] = sum p_c ; out_nll[r] = sum log p_{gt_r(v)}(v)
__global__ __launch_bounds__(256) void soft_metric_partial_kernel(const float* __restrict__ p, const uint8_t* __restrict__ gt,
                                                                  int C, int R, int64_t nvox, double* __restrict__ part) {
  // part [gridDim.x][R][C*3 + 1]
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int per = C * 3 + 1;
  for (int r = 0; r < R; ++r) {
    for (int k = 0; k < per; ++k) {
      const int c = k / 3, which = k - c * 3;
      double acc = 0.0;
      for (int64_t v = (int64_t)blockIdx.x * 256 + tid; v < nvox; v += (int64_t)gridDim.x * 256) {
        const int g = (int)gt[(size_t)r * nvox + v];
        if (k == per - 1) {
          if (g < C) acc += (double)logf(p[(size_t)g * nvox + v]);   // torch.log of the float32 probability
        } else if (which == 0) {
          if (g == c) acc += (double)p[(size_t)c * nvox + v];
        } else if (which == 1) {
          if (g == c) acc += 1.0;
        } else {
          acc += (double)p[(size_t)c * nvox + v];
        }
      }
      red[tid] = acc;
      __syncthreads();
      for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
      }
      if (tid == 0) part[((size_t)blockIdx.x * R + r) * per + k] = red[0];
      __syncthreads();
    }
  }
}

__global__ void soft_metric_final_kernel(const double* __restrict__ part, int nblocks, int n, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s += part[(size_t)b * n + i];   // fixed order
  out[i] = s;
}

extern "C" int64_t vx_soft_metric_workspace_bytes(int C, int R) {
  if (C <= 0 || R <= 0) return 0;
  return (int64_t)256 * R * (C * 3 + 1) * (int64_t)sizeof(double);
}

extern "C" int vx_soft_metric_sums(const float* prob, const uint8_t* gt, int C, int R, int64_t nvox, double* sums,
                                   void* workspace, vx_stream_t stream) {
  if (C <= 0 || C > 255 || R <= 0 || nvox <= 0) VX_FAIL(VX_E_SHAPE, "vx_soft_metric_sums: C=%d R=%d nvox=%lld", C, R, (long long)nvox);
  if (!prob || !gt || !sums || !workspace) VX_FAIL(VX_E_NULL, "vx_soft_metric_sums: null pointer");
  hipStream_t s = (hipStream_t)stream;
  int bx = (int)((nvox + 255) / 256);
  if (bx > 256) bx = 256;
  const int n = R * (C * 3 + 1);
  hipLaunchKernelGGL(soft_metric_partial_kernel, dim3(bx), dim3(256), 0, s, prob, gt, C, R, nvox, (double*)workspace);
  hipLaunchKernelGGL(soft_metric_final_kernel, dim3((n + 63) / 64), dim3(64), 0, s, (const double*)workspace, bx, n, sums);
  VX_CHECK_LAUNCH("vx_soft_metric_sums");
  return VX_OK;
}

// ---- vx_soft_metric_sums_batched: the same sums for the B volumes of a 3D inference step in ONE pass over the data ----------------
// (calculate_metrics of test_3D.py:537-575 runs calculate_test_metrics per case; the one-image kernel above walks the volume once
// per output scalar)
// An image is cut into spans of SMB_SPAN = 4096 voxels (a rule of nvox alone: image b of a batch is cut, summed and combined exactly
// as the same image submitted alone); a workgroup owns a span, a lane 4 tiles x 4 consecutive voxels of it:
//   1. the lane's labels of all R raters are loaded once, four to a register (one 32-bit load per rater and tile);
//   2. per class c the lane's 16 probabilities are loaded once (16-byte loads) and every sum that involves p_c is formed from those
//      registers: sum p_c (rater-independent: once), and per rater sum p_c [g_r = c] (float64), #[g_r = c] (an integer, counted as
//      one) and this class's share of sum logf(p_{g_r}) -- logf is taken once per (voxel, class) and selected per rater;
//   3. the lane partials of a class go down a fixed __shfl_down tree per wave, the four wave totals are added in wave order by one
//      thread per scalar, and the workgroup's partial lands in the workspace [B][spans][R][3C + 1] (sum p_c in rater 0's slot only);
//   4. a finalize launch adds an image's span partials in span order and replicates sum p_c into every rater's row.
// No atomics and no data-dependent order: bit-reproducible, and independent of B.  Labels >= C (255 included: also what a lane sees
// past the end of the image) match no class and take no log term.  Where nvox % 4 != 0 (or a base pointer is not aligned) the same
// lanes take the same voxels with scalar loads: the sums do not depend on which loads were used.
// Registers: RT = 4 holds the raters of the 3D data sets (R <= 4); RT = 31 is the general instance (one wave per SIMD).
constexpr int SMB_MAXC = 32, SMB_MAXR = 31;
constexpr int SMB_TILES = 4;
constexpr int SMB_SPAN = 256 * 4 * SMB_TILES;
constexpr int64_t SMB_MAXWG = 65536;   // workgroups of a launch; more spans than that: a workgroup takes every SMB_MAXWG-th

__device__ __forceinline__ f32x4 smb_load_p(const float* __restrict__ p, int64_t v, int64_t nvox, bool vec) {
  f32x4 q = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    if (v < nvox) q = *reinterpret_cast<const f32x4*>(p + v);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (v + j < nvox) q[j] = p[v + j];
  }
  return q;
}

__device__ __forceinline__ unsigned smb_load_g(const uint8_t* __restrict__ g, int64_t v, int64_t nvox, bool vec) {
  unsigned w = 0xffffffffu;
  if (vec) {
    if (v < nvox) w = *reinterpret_cast<const unsigned*>(g + v);
  } else {
    w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) w |= (v + j < nvox ? (unsigned)g[v + j] : 255u) << (8 * j);
  }
  return w;
}

// lane 0 ends with the wave's total; the tree is the same for every call
__device__ __forceinline__ double smb_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}
__device__ __forceinline__ int smb_wave_sum(int x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

template <int RT>
__global__ __launch_bounds__(256, RT <= 4 ? 4 : 1) void soft_metric_batched_kernel(const float* __restrict__ prob, const uint8_t* __restrict__ gt, int C,
                                                                  int R, int64_t nvox, int64_t nwg, int64_t nspan, int vec,
                                                                  double* __restrict__ part) {
  __shared__ double red[2][4][2 * RT + 1];   // [class parity][wave][sum p_c | sum p_c [g_r = c] | #[g_r = c]]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = 3 * C + 1;
  for (int64_t sp = blockIdx.x; sp < nspan; sp += gridDim.x) {   // span sp = image b, span blk of it
    const int64_t b = sp / nwg, blk = sp - b * nwg;
    const float* p = prob + (size_t)b * C * nvox;
    const uint8_t* g = gt + (size_t)b * R * nvox;
    double* o = part + (size_t)sp * R * per;
    const int64_t v0 = blk * SMB_SPAN + tid * 4;
    unsigned lab[RT][SMB_TILES];
    double nll[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      nll[r] = 0.0;
#pragma unroll
      for (int t = 0; t < SMB_TILES; ++t)
        lab[r][t] = r < R ? smb_load_g(g + (size_t)r * nvox, v0 + t * 1024, nvox, vec) : 0xffffffffu;
    }
    for (int c = 0; c < C; ++c) {
      f32x4 q[SMB_TILES], lq[SMB_TILES];
#pragma unroll
      for (int t = 0; t < SMB_TILES; ++t) q[t] = smb_load_p(p + (size_t)c * nvox, v0 + t * 1024, nvox, vec);
      double ps = 0.0;
#pragma unroll
      for (int t = 0; t < SMB_TILES; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ps += (double)q[t][j];
          lq[t][j] = logf(q[t][j]);   // torch.log of the float32 probability (past the end: log 0, never selected)
        }
      double* rd = red[c & 1][wave];
      ps = smb_wave_sum(ps);
      if (lane == 0) rd[0] = ps;
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        if (r < R) {
          double in = 0.0;
          int cn = 0;
#pragma unroll
          for (int t = 0; t < SMB_TILES; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const bool m = ((lab[r][t] >> (8 * j)) & 255u) == (unsigned)c;
              in += (double)(m ? q[t][j] : 0.f);
              nll[r] += (double)(m ? lq[t][j] : 0.f);
              cn += m ? 1 : 0;
            }
          in = smb_wave_sum(in);
          cn = smb_wave_sum(cn);
          if (lane == 0) {
            rd[1 + r] = in;
            rd[1 + RT + r] = (double)cn;
          }
        }
      }
      __syncthreads();
      // (the other parity is written next: its readers passed this barrier's predecessor)
      if (tid < 1 + 2 * RT) {
        const int r = tid == 0 ? 0 : (tid - 1) % RT, which = tid == 0 ? 2 : (tid <= RT ? 0 : 1);
        if (r < R) o[r * per + 3 * c + which] = ((red[c & 1][0][tid] + red[c & 1][1][tid]) + red[c & 1][2][tid]) + red[c & 1][3][tid];
      }
    }
    double* rd = red[C & 1][wave];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      if (r < R) {
        const double s = smb_wave_sum(nll[r]);
        if (lane == 0) rd[r] = s;
      }
    }
    __syncthreads();
    if (tid < R) o[tid * per + 3 * C] = ((red[C & 1][0][tid] + red[C & 1][1][tid]) + red[C & 1][2][tid]) + red[C & 1][3][tid];
    __syncthreads();   // the next span's first class may write the parity just read
  }
}

// sums[b][r][k] = the span partials of image b added in span order; sum p_c (k = 3c + 2) from rater 0's slot for every rater
__global__ __launch_bounds__(256) void soft_metric_batched_final_kernel(const double* __restrict__ part, int64_t n, int K, int per,
                                                                        int64_t nwg, double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / K;
    const int k = (int)(i - b * K), j = k % per;
    const double* p = part + (size_t)b * nwg * K + ((j < per - 1 && j % 3 == 2) ? j : k);
    double s = 0.0;
    for (int64_t blk = 0; blk < nwg; ++blk) s += p[(size_t)blk * K];
    out[i] = s;
  }
}

static bool smb_shape_ok(int B, int C, int R, int64_t nvox) {
  return B >= 1 && C >= 1 && C <= SMB_MAXC && R >= 1 && R <= SMB_MAXR && nvox >= 1 && nvox <= MAB_MAXVOX;
}

extern "C" int64_t vx_soft_metric_batched_workspace_bytes(int B, int C, int R, int64_t nvox) {
  if (!smb_shape_ok(B, C, R, nvox)) return 0;
  const int64_t nwg = (nvox + SMB_SPAN - 1) / SMB_SPAN;                     // <= 2^27
  const int64_t row = (int64_t)R * (3 * C + 1) * (int64_t)sizeof(double);   // < 2^15
  const int64_t nspan = (int64_t)B * nwg;                                   // < 2^58
  return nspan > INT64_MAX / row ? 0 : nspan * row;                         // (no such batch fits a device: 0, refused below)
}

extern "C" int vx_soft_metric_sums_batched(const float* prob, const uint8_t* gt, int B, int C, int R, int64_t nvox, double* sums,
                                           void* workspace, vx_stream_t stream) {
  if (!smb_shape_ok(B, C, R, nvox))
    VX_FAIL(VX_E_SHAPE, "vx_soft_metric_sums_batched: B=%d (>= 1) C=%d (1..%d) R=%d (1..%d) nvox=%lld (1..2^39)", B, C, SMB_MAXC, R,
            SMB_MAXR, (long long)nvox);
  if (vx_soft_metric_batched_workspace_bytes(B, C, R, nvox) == 0)
    VX_FAIL(VX_E_SHAPE, "vx_soft_metric_sums_batched: B=%d images of %lld voxels", B, (long long)nvox);
  if (!prob || !gt || !sums || !workspace) VX_FAIL(VX_E_NULL, "vx_soft_metric_sums_batched: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int64_t nwg = (nvox + SMB_SPAN - 1) / SMB_SPAN, nspan = (int64_t)B * nwg;
  const int vec = nvox % 4 == 0 && vx_aligned16(prob) && (((uintptr_t)gt) & 3u) == 0;
  const dim3 grid((unsigned)(nspan < SMB_MAXWG ? nspan : SMB_MAXWG));
  double* part = (double*)workspace;
  if (R <= 4)
    hipLaunchKernelGGL(soft_metric_batched_kernel<4>, grid, dim3(256), 0, s, prob, gt, C, R, nvox, nwg, nspan, vec, part);
  else
    hipLaunchKernelGGL(soft_metric_batched_kernel<SMB_MAXR>, grid, dim3(256), 0, s, prob, gt, C, R, nvox, nwg, nspan, vec, part);
  const int K = R * (3 * C + 1);
  const int64_t n = (int64_t)B * K, fb = (n + 255) / 256;
  hipLaunchKernelGGL(soft_metric_batched_final_kernel, dim3((unsigned)(fb < SMB_MAXWG ? fb : SMB_MAXWG)), dim3(256), 0, s,
                     (const double*)part, n, K, 3 * C + 1, nwg, sums);
  VX_CHECK_LAUNCH("vx_soft_metric_sums_batched");
  return VX_OK;
}
