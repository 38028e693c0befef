// Per-voxel reductions behind the evaluation stage's downstream scalars, each for a batch
// of images in one call; one image is a batch of one:
//   vx_ncc_batched         evaluation/metrics/ncc.py:9-25   the five sums compute_ncc derives its value from, both passes,
//                                                           the means formed on the device
//   vx_rater_variance      np.var(labels, axis=0) of R label volumes as a float64 map
//   vx_platt_sums_batched  evaluation/metrics/ace.py:13-41  Platt scaling (sklearn.calibration._sigmoid_calibration): the
//                                                           O(voxels) part of every optimiser step -- loss, gradient and
//                                                           Hessian sums of the two-parameter sigmoid fit, each item with
//                                                           its own (A, B, t_pos, t_neg)
//   vx_calib_bins_batched  evaluation/metrics/ace.py:44-90  platt_scale_confid + the 20-bin statistics of calib_stats
// All sums are float64 and DETERMINISTIC, formed with a fixed association --
//   thread t of block b adds elements b * 256 + t + k * 131072 in ascending k,
//   a 64-lane shuffle tree, the four waves of the block in order, the 512 block rows in index order --
// and the library is compiled with -ffp-contract=off: no multiply-add below is fused.
// Grid (EM_BLOCKS, n_items): block (b, i) runs block row b of item i into item i's partial rows; one workgroup per item
// then adds the rows in index order.  An item's numbers do not depend on its batch mates.  No atomics; nothing but the
// descriptor upload touches the host; no wait on the stream.
#include <string.h>

#include <vector>

#include "common.h"
#include "staging.h"

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
    if (prob != prob) bin = NB - 1;   // np.digitize(nan, bins) = len(bins): a NaN map value counts in bin 20, whose sum is NaN
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

namespace {
__global__ __launch_bounds__(EM_THREADS) void ncc_batched_kernel(const vx_ncc_item* __restrict__ items, int pass,
                                                                 const double* sums, double* __restrict__ partial) {
  const vx_ncc_item it = items[blockIdx.y];
  double* rows = partial + (size_t)blockIdx.y * EM_BLOCKS * 3;
  double mg = 0.0, mp = 0.0;
  if (pass == 1) {   // the host's s0[0] / n: one IEEE division of the pass-0 sum by the element count
    mg = sums[(size_t)blockIdx.y * 5 + 0] / (double)it.n_gt;
    mp = sums[(size_t)blockIdx.y * 5 + 1] / (double)it.n_gt;
  }
  if (it.gt_R > 0)
    em_ncc_body(em_var_src{(const int32_t*)it.gt, it.gt_R, it.n_gt}, it.pred, it.pred_dtype, it.n_gt, pass, mg, mp, rows);
  else
    em_ncc_body(em_map_src{it.gt, it.gt_dtype}, it.pred, it.pred_dtype, it.n_gt, pass, mg, mp, rows);
}

__global__ __launch_bounds__(EM_THREADS) void platt_batched_kernel(const PlattArgs* __restrict__ items, double* __restrict__ partial) {
  const PlattArgs a = items[blockIdx.y];
  em_platt_body(a, partial + (size_t)blockIdx.y * EM_BLOCKS * 8);
}

__global__ __launch_bounds__(EM_THREADS) void calib_bins_batched_kernel(const BinItem* __restrict__ items, BinEdges edges,
                                                                        double* __restrict__ partial) {
  const BinItem a = items[blockIdx.y];
  em_bins_body(a, edges, partial + (size_t)blockIdx.y * EM_BLOCKS * 3 * EM_NB);
}

// one workgroup per item: out[item * stride + off + k] = the item's EM_BLOCKS rows added in index order
__global__ __launch_bounds__(64) void em_final_batched_kernel(const double* __restrict__ partial, int K, double* __restrict__ out,
                                                              int stride, int off) {
  em_final_rows(partial + (size_t)blockIdx.x * EM_BLOCKS * K, EM_BLOCKS, K, out + (size_t)blockIdx.x * stride + off);
}

__global__ __launch_bounds__(256) void rater_variance_kernel(const int32_t* __restrict__ lab, int R, int64_t n, double* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = em_rater_var(lab, R, n, i);
}

// ---------------------------------------------------------------------------------------------------------------
// Argument checks and workspace layout: [descriptor table][n_items x EM_BLOCKS rows of K doubles].  Host code only.
struct em_plan {
  size_t table_bytes = 0, off_partial = 0, bytes = 0;
  char err[160] = {0};
};

int em_layout(const char* who, int n_items, size_t entry, int K, em_plan* p) {
  if (n_items < 1 || n_items > VX_EM_MAX_ITEMS) VX_REFUSE(p, VX_E_SHAPE, "%s: n_items %d outside 1..%d", who, n_items, VX_EM_MAX_ITEMS);
  p->table_bytes = (size_t)n_items * entry;
  p->off_partial = vx_align256(p->table_bytes);
  p->bytes = p->off_partial + (size_t)n_items * EM_BLOCKS * K * sizeof(double);
  return VX_OK;
}

int em_plan_raters(const char* who, const vx_em_item* items, int n_items, size_t entry, int K, em_plan* p) {
  if (!items) VX_REFUSE(p, VX_E_NULL, "%s: null items", who);
  const int rc = em_layout(who, n_items, entry, K, p);
  if (rc != VX_OK) return rc;
  for (int i = 0; i < n_items; ++i) {
    const vx_em_item& it = items[i];
    if (!it.unc || !it.ref || !it.pred) VX_REFUSE(p, VX_E_NULL, "%s: item %d: null map, reference or prediction", who, i);
    if (it.dtype != VX_F32 && it.dtype != VX_F64) VX_REFUSE(p, VX_E_DTYPE, "%s: item %d: dtype %d", who, i, it.dtype);
    if (it.R < 1 || it.nvox < 1 || it.nvox > INT64_MAX / it.R)
      VX_REFUSE(p, VX_E_SHAPE, "%s: item %d: R %d, nvox %lld", who, i, it.R, (long long)it.nvox);
  }
  return VX_OK;
}

int em_plan_ncc(const vx_ncc_item* items, int n_items, em_plan* p) {
  const char* who = "vx_ncc_batched";
  if (!items) VX_REFUSE(p, VX_E_NULL, "%s: null items", who);
  const int rc = em_layout(who, n_items, sizeof(vx_ncc_item), 3, p);
  if (rc != VX_OK) return rc;
  for (int i = 0; i < n_items; ++i) {
    const vx_ncc_item& it = items[i];
    if (!it.gt || !it.pred) VX_REFUSE(p, VX_E_NULL, "%s: item %d: null map", who, i);
    if (it.gt_R < 0) VX_REFUSE(p, VX_E_SHAPE, "%s: item %d: gt_R %d", who, i, it.gt_R);
    if ((it.gt_R == 0 && it.gt_dtype != VX_F32 && it.gt_dtype != VX_F64) || (it.pred_dtype != VX_F32 && it.pred_dtype != VX_F64))
      VX_REFUSE(p, VX_E_DTYPE, "%s: item %d: dtypes %d, %d", who, i, it.gt_dtype, it.pred_dtype);
    if (it.n_gt < 1 || it.n_pred < 1) VX_REFUSE(p, VX_E_SHAPE, "%s: item %d: empty map", who, i);
    if (it.n_gt != it.n_pred)
      VX_REFUSE(p, VX_E_SHAPE, "%s: item %d: maps of different size (%lld, %lld)", who, i, (long long)it.n_gt, (long long)it.n_pred);
    if (it.gt_R > 0 && it.n_gt > INT64_MAX / it.gt_R) VX_REFUSE(p, VX_E_SHAPE, "%s: item %d: gt_R %d x %lld", who, i, it.gt_R, (long long)it.n_gt);
  }
  return VX_OK;
}

int em_check_buffers(const char* who, const em_plan& p, const void* out, const void* workspace, size_t workspace_bytes) {
  if (!out || !workspace) VX_FAIL(VX_E_NULL, "%s: null out or workspace", who);
  if (workspace_bytes < p.bytes) VX_FAIL(VX_E_WORKSPACE, "%s: workspace needs %zu bytes", who, p.bytes);
  if (!vx_aligned16(workspace)) VX_FAIL(VX_E_ALIGN, "%s: workspace not 16-byte aligned", who);
  return VX_OK;
}

// the descriptor table goes up through the pinned staging buffer of staging.h: no wait on the stream
vx_staging g_stage;

int em_upload(const char* who, const void* table, size_t bytes, void* workspace, hipStream_t s) {
  const vx_stage_part part = {table, bytes, 0};
  return vx_staged_upload(g_stage, who, &part, 1, bytes, workspace, s);
}

em_raters em_raters_of(const vx_em_item& it, int ignore_value) {
  em_raters x;
  x.unc = it.unc; x.dtype = it.dtype; x.ref = it.ref; x.pred = it.pred; x.R = it.R; x.nvox = it.nvox; x.ignore_value = ignore_value;
  return x;
}
}  // namespace

extern "C" size_t vx_ncc_batched_workspace_bytes(const vx_ncc_item* items, int n_items) {
  em_plan p;
  return em_plan_ncc(items, n_items, &p) == VX_OK ? p.bytes : 0;
}

extern "C" int vx_ncc_batched(const vx_ncc_item* items, int n_items, double* sums, void* workspace, size_t workspace_bytes,
                              vx_stream_t stream) {
  const char* who = "vx_ncc_batched";
  em_plan p;
  int rc = em_plan_ncc(items, n_items, &p);
  if (rc != VX_OK) VX_FAIL(rc, "%s", p.err);
  if ((rc = em_check_buffers(who, p, sums, workspace, workspace_bytes)) != VX_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = em_upload(who, items, p.table_bytes, workspace, s)) != VX_OK) return rc;
  const vx_ncc_item* table = (const vx_ncc_item*)workspace;
  double* partial = (double*)((char*)workspace + p.off_partial);
  // (a pass-0 row is {sum gt, sum pred, 0}: its third number lands in sums[2], which pass 1 then overwrites)
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(ncc_batched_kernel, dim3(EM_BLOCKS, n_items), dim3(EM_THREADS), 0, s, table, pass, (const double*)sums, partial);
    hipLaunchKernelGGL(em_final_batched_kernel, dim3(n_items), dim3(64), 0, s, (const double*)partial, 3, sums, 5, pass == 0 ? 0 : 2);
  }
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}

extern "C" int vx_rater_variance(const int32_t* labels, int R, int64_t nvox, double* variance, vx_stream_t stream) {
  if (!labels || !variance) VX_FAIL(VX_E_NULL, "vx_rater_variance: null pointer");
  if (R < 1 || nvox < 1 || nvox > INT64_MAX / R) VX_FAIL(VX_E_SHAPE, "vx_rater_variance: R %d, nvox %lld", R, (long long)nvox);
  const int64_t blocks = (nvox + 255) / 256;
  hipLaunchKernelGGL(rater_variance_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, labels, R,
                     nvox, variance);
  VX_CHECK_LAUNCH("vx_rater_variance");
  return VX_OK;
}

extern "C" size_t vx_platt_batched_workspace_bytes(const vx_em_item* items, int n_items) {
  em_plan p;
  return em_plan_raters("vx_platt_sums_batched", items, n_items, sizeof(PlattArgs), 8, &p) == VX_OK ? p.bytes : 0;
}

extern "C" int vx_platt_sums_batched(const vx_em_item* items, int n_items, const double* params, int ignore_value, double* sums,
                                     void* workspace, size_t workspace_bytes, vx_stream_t stream) {
  const char* who = "vx_platt_sums_batched";
  em_plan p;
  int rc = em_plan_raters(who, items, n_items, sizeof(PlattArgs), 8, &p);
  if (rc != VX_OK) VX_FAIL(rc, "%s", p.err);
  if (!params) VX_FAIL(VX_E_NULL, "%s: null params", who);
  if ((rc = em_check_buffers(who, p, sums, workspace, workspace_bytes)) != VX_OK) return rc;
  std::vector<PlattArgs> table((size_t)n_items);
  for (int i = 0; i < n_items; ++i) {
    PlattArgs& a = table[i];
    memset(&a, 0, sizeof(a));
    a.x = em_raters_of(items[i], ignore_value);
    a.A = params[4 * i]; a.B = params[4 * i + 1]; a.t_pos = params[4 * i + 2]; a.t_neg = params[4 * i + 3];
  }
  hipStream_t s = (hipStream_t)stream;
  if ((rc = em_upload(who, table.data(), p.table_bytes, workspace, s)) != VX_OK) return rc;
  double* partial = (double*)((char*)workspace + p.off_partial);
  hipLaunchKernelGGL(platt_batched_kernel, dim3(EM_BLOCKS, n_items), dim3(EM_THREADS), 0, s, (const PlattArgs*)workspace, partial);
  hipLaunchKernelGGL(em_final_batched_kernel, dim3(n_items), dim3(64), 0, s, (const double*)partial, 8, sums, 8, 0);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}

extern "C" size_t vx_calib_batched_workspace_bytes(const vx_em_item* items, int n_items) {
  em_plan p;
  return em_plan_raters("vx_calib_bins_batched", items, n_items, sizeof(BinItem), 3 * EM_NB, &p) == VX_OK ? p.bytes : 0;
}

extern "C" int vx_calib_bins_batched(const vx_em_item* items, int n_items, const double* ab, const double* edges21, int ignore_value,
                                     double* bins63, void* workspace, size_t workspace_bytes, vx_stream_t stream) {
  const char* who = "vx_calib_bins_batched";
  em_plan p;
  int rc = em_plan_raters(who, items, n_items, sizeof(BinItem), 3 * EM_NB, &p);
  if (rc != VX_OK) VX_FAIL(rc, "%s", p.err);
  if (!ab || !edges21) VX_FAIL(VX_E_NULL, "%s: null parameters or edges", who);
  if ((rc = em_check_buffers(who, p, bins63, workspace, workspace_bytes)) != VX_OK) return rc;
  std::vector<BinItem> table((size_t)n_items);
  for (int i = 0; i < n_items; ++i) {
    BinItem& a = table[i];
    memset(&a, 0, sizeof(a));
    a.x = em_raters_of(items[i], ignore_value);
    a.A = ab[2 * i]; a.B = ab[2 * i + 1];
  }
  BinEdges e;
  for (int k = 0; k < EM_NB; ++k) e.e[k] = edges21[k];   // HOST array (np.linspace, bit for bit the reference's edges)
  hipStream_t s = (hipStream_t)stream;
  if ((rc = em_upload(who, table.data(), p.table_bytes, workspace, s)) != VX_OK) return rc;
  double* partial = (double*)((char*)workspace + p.off_partial);
  hipLaunchKernelGGL(calib_bins_batched_kernel, dim3(EM_BLOCKS, n_items), dim3(EM_THREADS), 0, s, (const BinItem*)workspace, e, partial);
  hipLaunchKernelGGL(em_final_batched_kernel, dim3(n_items), dim3(64), 0, s, (const double*)partial, 3 * EM_NB, bins63, 3 * EM_NB, 0);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}
