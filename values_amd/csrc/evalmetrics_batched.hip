// The per-voxel reductions of evalmetrics.hip for a batch of images in one call:
//   vx_ncc_batched         the five sums compute_ncc derives its value from, both passes, the means formed on the device
//   vx_rater_variance      np.var(labels, axis=0) of R label volumes as a float64 map
//   vx_platt_sums_batched  the eight sums of vx_platt_sums per item, each item with its own (A, B, t_pos, t_neg)
//   vx_calib_bins_batched  the 63 numbers of vx_calib_bins per item
// Grid (EM_BLOCKS, n_items): block (b, i) is block b of item i's per-image launch and runs the same body
// (evalmetrics_core.h) into item i's partial rows; one workgroup per item then adds the rows in index order.  Every sum
// keeps the per-image association, so an item's numbers are the per-image entry points' bit for bit and do not depend on
// its batch mates.  No atomics; nothing but the descriptor upload touches the host; no wait on the stream.
#include <string.h>

#include <vector>

#include "evalmetrics_core.h"
#include "staging.h"

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

#define EM_REFUSE(code, ...)                       \
  do {                                             \
    snprintf(p->err, sizeof(p->err), __VA_ARGS__); \
    return (code);                                 \
  } while (0)

int em_layout(const char* who, int n_items, size_t entry, int K, em_plan* p) {
  if (n_items < 1 || n_items > VX_EM_MAX_ITEMS) EM_REFUSE(VX_E_SHAPE, "%s: n_items %d outside 1..%d", who, n_items, VX_EM_MAX_ITEMS);
  p->table_bytes = (size_t)n_items * entry;
  p->off_partial = vx_align256(p->table_bytes);
  p->bytes = p->off_partial + (size_t)n_items * EM_BLOCKS * K * sizeof(double);
  return VX_OK;
}

int em_plan_raters(const char* who, const vx_em_item* items, int n_items, size_t entry, int K, em_plan* p) {
  if (!items) EM_REFUSE(VX_E_NULL, "%s: null items", who);
  const int rc = em_layout(who, n_items, entry, K, p);
  if (rc != VX_OK) return rc;
  for (int i = 0; i < n_items; ++i) {
    const vx_em_item& it = items[i];
    if (!it.unc || !it.ref || !it.pred) EM_REFUSE(VX_E_NULL, "%s: item %d: null map, reference or prediction", who, i);
    if (it.dtype != VX_F32 && it.dtype != VX_F64) EM_REFUSE(VX_E_DTYPE, "%s: item %d: dtype %d", who, i, it.dtype);
    if (it.R < 1 || it.nvox < 1 || it.nvox > INT64_MAX / it.R)
      EM_REFUSE(VX_E_SHAPE, "%s: item %d: R %d, nvox %lld", who, i, it.R, (long long)it.nvox);
  }
  return VX_OK;
}

int em_plan_ncc(const vx_ncc_item* items, int n_items, em_plan* p) {
  const char* who = "vx_ncc_batched";
  if (!items) EM_REFUSE(VX_E_NULL, "%s: null items", who);
  const int rc = em_layout(who, n_items, sizeof(vx_ncc_item), 3, p);
  if (rc != VX_OK) return rc;
  for (int i = 0; i < n_items; ++i) {
    const vx_ncc_item& it = items[i];
    if (!it.gt || !it.pred) EM_REFUSE(VX_E_NULL, "%s: item %d: null map", who, i);
    if (it.gt_R < 0) EM_REFUSE(VX_E_SHAPE, "%s: item %d: gt_R %d", who, i, it.gt_R);
    if ((it.gt_R == 0 && it.gt_dtype != VX_F32 && it.gt_dtype != VX_F64) || (it.pred_dtype != VX_F32 && it.pred_dtype != VX_F64))
      EM_REFUSE(VX_E_DTYPE, "%s: item %d: dtypes %d, %d", who, i, it.gt_dtype, it.pred_dtype);
    if (it.n_gt < 1 || it.n_pred < 1) EM_REFUSE(VX_E_SHAPE, "%s: item %d: empty map", who, i);
    if (it.n_gt != it.n_pred)
      EM_REFUSE(VX_E_SHAPE, "%s: item %d: maps of different size (%lld, %lld)", who, i, (long long)it.n_gt, (long long)it.n_pred);
    if (it.gt_R > 0 && it.n_gt > INT64_MAX / it.gt_R) EM_REFUSE(VX_E_SHAPE, "%s: item %d: gt_R %d x %lld", who, i, it.gt_R, (long long)it.n_gt);
  }
  return VX_OK;
}
#undef EM_REFUSE

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
