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
