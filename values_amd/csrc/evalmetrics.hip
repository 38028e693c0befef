// Per-voxel reductions behind the evaluation stage's downstream scalars:
//   vx_ncc_sums     evaluation/metrics/ncc.py:9-25       normalised cross correlation of two uncertainty maps
//   vx_platt_sums   evaluation/metrics/ace.py:13-41      Platt scaling (sklearn.calibration._sigmoid_calibration): the
//                                                        O(voxels) part of every optimiser step -- loss, gradient and
//                                                        Hessian sums of the two-parameter sigmoid fit
//   vx_calib_bins   evaluation/metrics/ace.py:44-90      platt_scale_confid + the 20-bin statistics of calib_stats
// All sums are float64 and DETERMINISTIC: a fixed grid of workgroups leaves one partial row each, a single workgroup
// adds the rows in index order (no atomics), so a rerun gives the same bits.
// "correct" follows ace.py:27-29 / :112-114: the mean prediction compared with each of the R reference segmentations
// (rater_correct = reference_segs == pred_seg, the map repeated per rater), voxels whose reference equals
// ignore_value dropped (ignore_value < 0: none).
#include "evalmetrics_core.h"

// the grid walk, the per-element arithmetic and the reductions are evalmetrics_core.h's, shared with the batched kernels
namespace {
constexpr int NB = EM_NB;

__global__ __launch_bounds__(256) void em_final_kernel(const double* __restrict__ partial, int nblocks, int K,
                                                       double* __restrict__ out) {
  em_final_rows(partial, nblocks, K, out);
}

__global__ __launch_bounds__(EM_THREADS) void ncc_kernel(const void* __restrict__ g, int gd, const void* __restrict__ p, int pd,
                                                         int64_t n, int pass, double mg, double mp,
                                                         double* __restrict__ partial) {
  em_ncc_body(em_map_src{g, gd}, p, pd, n, pass, mg, mp, partial);
}

__global__ __launch_bounds__(EM_THREADS) void platt_kernel(PlattArgs a, double* __restrict__ partial) { em_platt_body(a, partial); }

struct BinArgs {
  BinItem it;
  BinEdges edges;
};

__global__ __launch_bounds__(EM_THREADS) void calib_bins_kernel(BinArgs a, double* __restrict__ partial) {
  em_bins_body(a.it, a.edges, partial);
}
}  // namespace

extern "C" int64_t vx_evalmetrics_workspace_bytes(void) { return (int64_t)EM_BLOCKS * 3 * NB * sizeof(double); }

extern "C" int vx_ncc_sums(const void* gt, int gt_dtype, const void* pred, int pred_dtype, int64_t n, int pass, double mean_gt,
                           double mean_pred, double* sums, void* workspace, vx_stream_t stream) {
  if (!gt || !pred || !sums || !workspace) VX_FAIL(VX_E_NULL, "vx_ncc_sums: null pointer");
  if (n <= 0) VX_FAIL(VX_E_SHAPE, "vx_ncc_sums: empty map");
  if ((gt_dtype != VX_F32 && gt_dtype != VX_F64) || (pred_dtype != VX_F32 && pred_dtype != VX_F64) || (pass != 0 && pass != 1))
    VX_FAIL(VX_E_DTYPE, "vx_ncc_sums: dtype / pass");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ncc_kernel, dim3(EM_BLOCKS), dim3(EM_THREADS), 0, s, gt, gt_dtype, pred, pred_dtype, n, pass, mean_gt,
                     mean_pred, (double*)workspace);
  hipLaunchKernelGGL(em_final_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, EM_BLOCKS, 3, sums);
  VX_CHECK_LAUNCH("vx_ncc_sums");
  return VX_OK;
}

extern "C" int vx_platt_sums(const void* unc, int dtype, const int32_t* ref, const int32_t* pred, int R, int64_t nvox,
                             int ignore_value, double A, double B, double t_pos, double t_neg, double* sums, void* workspace,
                             vx_stream_t stream) {
  if (!unc || !ref || !pred || !sums || !workspace) VX_FAIL(VX_E_NULL, "vx_platt_sums: null pointer");
  if (R <= 0 || nvox <= 0) VX_FAIL(VX_E_SHAPE, "vx_platt_sums: empty input");
  if (dtype != VX_F32 && dtype != VX_F64) VX_FAIL(VX_E_DTYPE, "vx_platt_sums: dtype %d", dtype);
  PlattArgs a;
  a.x.unc = unc; a.x.dtype = dtype; a.x.ref = ref; a.x.pred = pred; a.x.R = R; a.x.nvox = nvox; a.x.ignore_value = ignore_value;
  a.A = A; a.B = B; a.t_pos = t_pos; a.t_neg = t_neg;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(platt_kernel, dim3(EM_BLOCKS), dim3(EM_THREADS), 0, s, a, (double*)workspace);
  hipLaunchKernelGGL(em_final_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, EM_BLOCKS, 8, sums);
  VX_CHECK_LAUNCH("vx_platt_sums");
  return VX_OK;
}

extern "C" int vx_calib_bins(const void* unc, int dtype, const int32_t* ref, const int32_t* pred, int R, int64_t nvox,
                             int ignore_value, double A, double B, const double* edges21, double* bins63, void* workspace,
                             vx_stream_t stream) {
  if (!unc || !ref || !pred || !edges21 || !bins63 || !workspace) VX_FAIL(VX_E_NULL, "vx_calib_bins: null pointer");
  if (R <= 0 || nvox <= 0) VX_FAIL(VX_E_SHAPE, "vx_calib_bins: empty input");
  if (dtype != VX_F32 && dtype != VX_F64) VX_FAIL(VX_E_DTYPE, "vx_calib_bins: dtype %d", dtype);
  BinArgs a;
  a.it.x.unc = unc; a.it.x.dtype = dtype; a.it.x.ref = ref; a.it.x.pred = pred; a.it.x.R = R; a.it.x.nvox = nvox;
  a.it.x.ignore_value = ignore_value;
  a.it.A = A; a.it.B = B;
  for (int k = 0; k < NB; ++k) a.edges.e[k] = edges21[k];   // HOST array (np.linspace, bit for bit the reference's edges)
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(calib_bins_kernel, dim3(EM_BLOCKS), dim3(EM_THREADS), 0, s, a, (double*)workspace);
  hipLaunchKernelGGL(em_final_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, EM_BLOCKS, 3 * NB, bins63);
  VX_CHECK_LAUNCH("vx_calib_bins");
  return VX_OK;
}
