// The per-voxel reductions of evalmetrics.hip (one image per call) and evalmetrics_batched.hip (a batch of images per
// call) as ONE source text: the grid walk, the per-element arithmetic and every level of the reduction.  A sum is formed
// with a fixed association --
//   thread t of block b adds elements b * 256 + t + k * 131072 in ascending k,
//   a 64-lane shuffle tree, the four waves of the block in order, the 512 block rows in index order --
// so a kernel that calls these bodies with blockIdx.x = block row and its own partial rows gives the per-image bits,
// whatever else its grid holds.  The library is compiled with -ffp-contract=off: no multiply-add below is fused.
#pragma once
#include "common.h"

constexpr int EM_BLOCKS = 512;
constexpr int EM_THREADS = 256;
constexpr int EM_NB = 21;   // len(bins) of calib_stats: np.linspace(0, 1 + 1e-8, 21); bincount(minlength = 21)

// `partial`: the EM_BLOCKS rows of K doubles of THIS reduction; block blockIdx.x writes its row
template <int K>
__device__ __forceinline__ void em_block_reduce(double (&v)[K], double* __restrict__ partial) {
  __shared__ double s_red[EM_THREADS / 64][K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double x = v[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_down(x, off, 64);
    if (lane == 0) s_red[wave][k] = x;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < EM_THREADS / 64; ++w) t += s_red[w][threadIdx.x];
    partial[(size_t)blockIdx.x * K + threadIdx.x] = t;
  }
}

// thread k < K adds the rows of one reduction in index order
__device__ __forceinline__ void em_final_rows(const double* __restrict__ partial, int nblocks, int K, double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= K) return;
  double t = 0.0;
  for (int b = 0; b < nblocks; ++b) t += partial[(size_t)b * K + k];
  out[k] = t;
}

__device__ __forceinline__ double em_load(const void* p, int dtype, int64_t i) {
  return dtype == VX_F64 ? reinterpret_cast<const double*>(p)[i] : (double)reinterpret_cast<const float*>(p)[i];
}

// ground-truth side of the NCC: a stored map ...
struct em_map_src {
  const void* p; int dtype;
  __device__ __forceinline__ double operator()(int64_t i) const { return em_load(p, dtype, i); }
};

// ... or np.var(labels, axis=0) of R int32 label volumes [R][n], evaluated per voxel in float64 in numpy's order (_var of
// numpy/core/_methods.py for integer input: sum over the raters in index order, / R, sum of (x - mean)^2 in index order, / R)
__device__ __forceinline__ double em_rater_var(const int32_t* __restrict__ lab, int R, int64_t n, int64_t i) {
  double s = 0.0;
  for (int r = 0; r < R; ++r) s += (double)lab[(int64_t)r * n + i];
  const double mean = s / (double)R;
  double q = 0.0;
  for (int r = 0; r < R; ++r) {
    const double d = (double)lab[(int64_t)r * n + i] - mean;
    q += d * d;
  }
  return q / (double)R;
}
struct em_var_src {
  const int32_t* lab; int R; int64_t n;
  __device__ __forceinline__ double operator()(int64_t i) const { return em_rater_var(lab, R, n, i); }
};

// pass 0: sum g, sum p.   pass 1 (means given): sum (g - mg)^2, sum (p - mp)^2, sum (g - mg)(p - mp)
template <class G>
__device__ __forceinline__ void em_ncc_body(const G& g, const void* __restrict__ p, int pd, int64_t n, int pass, double mg,
                                            double mp, double* __restrict__ partial) {
  double v[3] = {0.0, 0.0, 0.0};
  for (int64_t i = blockIdx.x * (int64_t)EM_THREADS + threadIdx.x; i < n; i += (int64_t)EM_BLOCKS * EM_THREADS) {
    const double a = g(i), b = em_load(p, pd, i);
    if (pass == 0) {
      v[0] += a;
      v[1] += b;
    } else {
      const double da = a - mg, db = b - mp;
      v[0] += da * da;
      v[1] += db * db;
      v[2] += da * db;
    }
  }
  em_block_reduce<3>(v, partial);
}

// one image of the calibration kernels: "correct" follows ace.py:27-29 / :112-114 (the mean prediction compared with each
// of the R reference segmentations, voxels whose reference equals ignore_value dropped; ignore_value < 0: none)
struct em_raters {
  const void* unc; int dtype;
  const int32_t* ref; const int32_t* pred;
  int R; int64_t nvox; int ignore_value;
};

struct PlattArgs {
  em_raters x;
  double A, B, t_pos, t_neg;
};

// out[0] valid voxels (over all raters), out[1] correct ones, out[2] loss, out[3] dA, out[4] dB,
// out[5] sum w F^2, out[6] sum w F, out[7] sum w      (w = P (1 - P); F = -unc as ace.py:32-34 passes it)
__device__ __forceinline__ void em_platt_body(const PlattArgs& a, double* __restrict__ partial) {
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t total = (int64_t)a.x.R * a.x.nvox;
  for (int64_t i = blockIdx.x * (int64_t)EM_THREADS + threadIdx.x; i < total; i += (int64_t)EM_BLOCKS * EM_THREADS) {
    const int64_t vx = i % a.x.nvox;
    const int ref = a.x.ref[i];
    if (a.x.ignore_value >= 0 && ref == a.x.ignore_value) continue;
    const bool correct = ref == a.x.pred[vx];
    const double F = -em_load(a.x.unc, a.x.dtype, vx);
    const double T = correct ? a.t_pos : a.t_neg;
    // P = expit(-(A F + B));  loss = -(T log P + (1 - T) log(1 - P)) in the overflow-free form of Platt's pseudo-code
    const double z = a.A * F + a.B;
    double P, loss;
    if (z >= 0) {
      const double e = exp(-z);
      P = e / (1.0 + e);
      loss = T * z + log1p(e);
    } else {
      const double e = exp(z);
      P = 1.0 / (1.0 + e);
      loss = (T - 1.0) * z + log1p(e);
    }
    const double d = T - P, w = P * (1.0 - P);
    v[0] += 1.0;
    v[1] += correct ? 1.0 : 0.0;
    v[2] += loss;
    v[3] += d * F;
    v[4] += d;
    v[5] += w * F * F;
    v[6] += w * F;
    v[7] += w;
  }
  em_block_reduce<8>(v, partial);
}

struct BinItem {
  em_raters x;
  double A, B;
};
struct BinEdges {
  double e[EM_NB];
};

// per workgroup: bin_sums[21], bin_true[21], bin_total[21] -> partial row of 63 doubles
__device__ __forceinline__ void em_bins_body(const BinItem& a, const BinEdges& edges, double* __restrict__ partial) {
  constexpr int NB = EM_NB;
  __shared__ double s_h[EM_THREADS / 64][3 * NB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // per-lane private histograms would need 63 registers of doubles; instead every lane walks its elements and the wave
  // combines bin by bin with a ballot-free masked reduction: 21 bins x 3 values, all lanes take part (deterministic order)
  double hs[NB], ht[NB], hc[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) { hs[k] = 0.0; ht[k] = 0.0; hc[k] = 0.0; }
  const int64_t total = (int64_t)a.x.R * a.x.nvox;
  for (int64_t i = blockIdx.x * (int64_t)EM_THREADS + threadIdx.x; i < total; i += (int64_t)EM_BLOCKS * EM_THREADS) {
    const int64_t vx = i % a.x.nvox;
    const int ref = a.x.ref[i];
    if (a.x.ignore_value >= 0 && ref == a.x.ignore_value) continue;
    const double conf = -em_load(a.x.unc, a.x.dtype, vx);             // uncalib_confid = -unc  (ace.py:117-121)
    const double prob = 1.0 / (1.0 + exp(conf * a.A + a.B));          // platt_scale_confid (ace.py:44-48)
    int bin = -1;                                                     // np.digitize(prob, bins) - 1
#pragma unroll
    for (int k = 0; k < NB; ++k) bin += (edges.e[k] <= prob) ? 1 : 0;
    const double corr = ref == a.x.pred[vx] ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const bool hit = bin == k;
      hs[k] += hit ? prob : 0.0;
      ht[k] += hit ? corr : 0.0;
      hc[k] += hit ? 1.0 : 0.0;
    }
  }
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    double x = hs[k], y = ht[k], z = hc[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      x += __shfl_down(x, off, 64);
      y += __shfl_down(y, off, 64);
      z += __shfl_down(z, off, 64);
    }
    if (lane == 0) { s_h[wave][k] = x; s_h[wave][NB + k] = y; s_h[wave][2 * NB + k] = z; }
  }
  __syncthreads();
  if (threadIdx.x < 3 * NB) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < EM_THREADS / 64; ++w) t += s_h[w][threadIdx.x];
    partial[(size_t)blockIdx.x * 3 * NB + threadIdx.x] = t;
  }
}
